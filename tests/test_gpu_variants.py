"""Every rollout kernel family the dispatcher can pick (plan_call / pick_family in csrc/sgym_hip.hip; launched by
launch_variant / launch_queue / launch_sliced / launch_wide), reached on purpose through each host entry point that can reach
it, and checked against the CPU oracle.

VARIANTS is a plain table: a batch recipe, the knobs that steer the dispatcher to the family, the entry point
(sg_rollout, sg_step with actions, sg_tick) and the exact sg_last_kernel() string.  Each GPU row asserts the name and
compares the final state, metric rows, events (and for RSS rows the four RSSDistances records) with the oracle on a few
scenarios spread over the batch: replayed and controlled lanes bit for bit (compare_final), collisions and events exact.

test_every_reported_kernel_has_a_row (CPU) reads every format string passed to note_kernel() and fails for a family
without a row.  test_reused_handle_equals_fresh_handle drives one handle through uploads that change the variant.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISPATCH_SRC = os.path.join(ROOT, "scenario_gym_amd", "csrc", "sgym_hip.hip")

WIDE = "sg::wide_move_kernel + wide_commit_kernel + wide_collide_kernel + wide_finish_kernel"
NO_TAB = dict(tab_min_steps=1000)            # every call below tab_min: no table variant
TAB = dict(tab_min_steps=1, chunk_steps=16)  # the table path, several chunks
DT = 1 / 30
# (n_entities, tile lanes G, wavefronts per scenario WV, scenarios): one row per tile shape of the general families
SHAPES = [(3, 4, 1, 32), (6, 8, 1, 24), (12, 16, 1, 16), (24, 32, 1, 12), (48, 64, 1, 8), (100, 64, 2, 6), (200, 64, 4, 4),
          (300, 64, 8, 3)]
ENTRIES = ("rollout", "step", "tick")


def _row(family, recipe, E, R, entry, expect, T=None, rss=False, road=False, tuning=None, slicing=False, env=None, models=False):
    T = T if T is not None else (10 if entry == "tick" else 16)
    rid = f"{family}-{recipe}-E{E}-{entry}" + ("-rss" if rss else "") + ("-road" if road else "")
    return dict(id=rid, family=family, recipe=recipe, E=E, R=R, T=T, entry=entry, rss=rss, road=road,
                tuning=NO_TAB if tuning is None else tuning, slicing=slicing, env=env or {}, models=models, expect=expect)


def _variants():
    rows = []
    for E, G, WV, R in SHAPES:
        Gp = max(G, 16)  # pedestrian agents are compiled for tiles of >= 16 lanes: sg_upload promotes narrower tiles
        for entry in ENTRIES:
            rows.append(_row("plain", "vehicle", E, R, entry, f"sg::rollout_kernel<{G}, {WV}, false, false>"))
            rows.append(_row("ped", "mixed", E, R, entry, f"sg::rollout_kernel<{Gp}, {WV}, true, false>"))
            rows.append(_row("rss", "vehicle", E, R, entry, f"sg::rollout_kernel_rss<{G}, {WV}>", rss=True))
            rows.append(_row("road", "pid", E, R, entry, f"sg::rollout_kernel_road<{G}, {WV}>", road=True))
            if WV < 8:
                rows.append(_row("rss_ped", "mixed", E, R, entry, f"sg::rollout_kernel_rss_ped<{Gp}, {WV}>", rss=True))
                rows.append(_row("rss_road", "vehicle", E, R, entry, f"sg::rollout_kernel_rss_road<{G}, {WV}>", rss=True, road=True))
            else:  # 257..512 entities: no fused variant carries RSS with pedestrians / ego_off_road, rss_kernel runs behind the step
                rows.append(_row("ped+rss", "mixed", E, R, entry, "sg::rollout_kernel<64, 8, true, false>", rss=True))
                rows.append(_row("road+rss", "vehicle", E, R, entry, "sg::rollout_kernel_road<64, 8>", rss=True, road=True))
                rows.append(_row("ped+road+rss", "mixed", E, R, entry, "sg::rollout_kernel<64, 8, true, false>", rss=True, road=True))
        if WV in (1, 2, 8):  # pedestrian agents + ego_off_road: ego_off_road_kernel behind every step of the pedestrian variant
            rows.append(_row("ped+road", "mixed", E, R, "rollout", f"sg::rollout_kernel<{Gp}, {WV}, true, false>", road=True))
        if WV < 8:  # the table path (calls of at least tab_min steps; sg_tick never takes it)
            for entry in ("rollout", "step"):
                rows.append(_row("tab_rows", "replay" if WV == 1 else "pid", E, R, entry, f"sg::rollout_kernel<{G}, {WV}, false, true>",
                                 T=40, tuning=TAB))
        if WV == 1:
            for entry in ("rollout", "step"):
                rows.append(_row("tab_planar", "pid_sparse", E, R, entry, f"sg::rollout_kernel_tab_planar<{G}>", T=40, tuning=TAB,
                                 env=dict(SG_QUEUE="0")))
                rows.append(_row("tab", "pid_sparse", E, R, entry, f"sg::rollout_kernel_tab<{G}>", T=40, tuning=TAB,
                                 env=dict(SG_QUEUE="0", SG_PLANAR="0")))
            rows.append(_row("tabq_planar", "pid_sparse", E, R, "rollout", f"sg::rollout_kernel_tabq_planar<{G}>", T=40, tuning=TAB))
            rows.append(_row("rss_tab", "pid", E, R, "rollout", f"sg::rollout_kernel_rss_tab<{G}>", T=40, rss=True, tuning=TAB,
                             env=dict(SG_QUEUE="0")))
            rows.append(_row("rss_tabq", "pid", E, R, "rollout", f"sg::rollout_kernel_rss_tabq<{G}>", T=40, rss=True, tuning=TAB))
            rows.append(_row("slice", "replay", E, R, "rollout", f"sg::rollout_kernel_slice<{G}>", T=40, tuning={}, slicing="always"))
            rows.append(_row("slice_tab", "pid_sparse", E, R, "rollout", f"sg::rollout_kernel_slice_tab<{G}>", T=40, tuning={},
                             slicing="always"))
    for E, G, entry in ((6, 8, "step"), (48, 64, "step")):
        rows.append(_row("tabq", "pid_sparse", E, 24, entry, f"sg::rollout_kernel_tabq<{G}>", T=40, tuning=TAB, env=dict(SG_PLANAR="0")))
        rows.append(_row("rss_tabq", "pid", E, 24, entry, f"sg::rollout_kernel_rss_tabq<{G}>", T=40, rss=True, tuning=TAB))
        rows.append(_row("rss_tab", "pid", E, 24, entry, f"sg::rollout_kernel_rss_tab<{G}>", T=40, rss=True, tuning=TAB,
                         env=dict(SG_QUEUE="0")))
    for E, WV, R in ((48, 1, 8), (100, 2, 6), (200, 4, 4)):  # the crowd kernels: all-pedestrian 64-lane tiles
        for entry in ENTRIES:
            rows.append(_row("crowd", "crowd", E, R, entry, f"sg::rollout_kernel_crowd<{WV}>"))
            rows.append(_row("crowd_models", "crowd", E, R, entry, f"sg::rollout_kernel_crowd_models<{WV}>", models=True))
        for entry in ("rollout", "step"):
            rows.append(_row("crowd_riders", "mixed", E, R, entry, f"sg::rollout_kernel_crowd_riders<{WV}>", T=40, tuning=TAB))
    for entry in ENTRIES:  # more than 512 entities: the multi-kernel step
        rows.append(_row("wide", "vehicle", 600, 2, entry, WIDE, T=8))
        rows.append(_row("wide", "mixed", 600, 2, entry, WIDE, T=8, rss=True))
    rows.append(_row("wide", "pid", 600, 2, "rollout", WIDE, T=8, road=True))
    return rows


VARIANTS = _variants()


# ------------------------------------------------------------------------------------------------ CPU: name coverage
def _note_kernel_formats(src):
    """Every string literal inside the argument list of a note_kernel( call (both arms of a ?: included)."""
    out = []
    for m in re.finditer(r"\bnote_kernel\(", src):
        i, depth = m.end(), 1
        while depth and i < len(src):
            c = src[i]
            if c == '"':
                j = i + 1
                while src[j] != '"':
                    j += 2 if src[j] == "\\" else 1
                out.append(src[i + 1:j])
                i = j
            elif c == "(":
                depth += 1
            elif c == ")":
                depth -= 1
            i += 1
    return out


def _format_regex(fmt):
    return re.compile("".join(r"\d+" if p == "%d" else re.escape(p) for p in re.split(r"(%d)", fmt)))


def uncovered_formats(rows, src):
    names = [r["expect"] for r in rows]
    return [f for f in dict.fromkeys(_note_kernel_formats(src)) if not any(_format_regex(f).fullmatch(n) for n in names)]


def test_every_reported_kernel_has_a_row():
    """A family the dispatcher can report (note_kernel) without a row of VARIANTS fails here, on the CPU."""
    with open(DISPATCH_SRC) as f:
        src = f.read()
    fmts = _note_kernel_formats(src)
    assert len(set(fmts)) >= 23, sorted(set(fmts))  # (the parse found the dispatcher's names)
    assert WIDE in fmts
    missing = uncovered_formats(VARIANTS, src)
    assert not missing, f"kernel families without a row in VARIANTS: {missing}"
    # ... and the check does bite: without the rows of one family, that family is named
    for fam in ("rss_tab", "crowd_models", "slice"):
        gone = uncovered_formats([r for r in VARIANTS if r["family"] != fam], src)
        assert gone and all(fam.split("_")[0] in g for g in gone), (fam, gone)
    ids = [r["id"] for r in VARIANTS]
    assert len(ids) == len(set(ids))


def test_rows_are_consistent():
    """Tile shapes the rows claim follow sg_create's rule; pedestrian rows below 16 lanes expect the promoted tile."""
    for r in VARIANTS:
        E = r["E"]
        G = 4
        while G < E and G < 64:
            G <<= 1
        m = re.search(r"<(\d+)", r["expect"])
        if r["family"] == "wide":
            assert E > 512
            continue
        if r["family"].startswith("crowd"):
            continue
        got = int(m.group(1))
        assert got == (max(G, 16) if r["recipe"] == "mixed" else G), r["id"]
        if r["entry"] == "tick":
            assert not any(t in r["expect"] for t in ("tab", "slice", "true>", "riders")), r["id"]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sga():
    import scenario_gym_amd as sga
    import scenario_gym_amd._lib as L

    L.load()
    return sga


def _nets(seed):
    """Random polygon road networks (the scene of test_rss_inside_pedestrian_and_off_road_rollouts): egos leave the road at
    different times."""
    rng = np.random.default_rng(seed)
    nets = []
    for n in range(3):
        rings = []
        for q in range(6):
            c = rng.uniform(-30, 30, 2)
            ang = np.sort(rng.uniform(0, 2 * np.pi, 12))
            rings.append(c + (rng.uniform(25, 50) * rng.uniform(0.7, 1.0, 12))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))
        vert_off = np.concatenate([[0], np.cumsum([len(r) for r in rings])])
        nets.append(dict(ring_off=np.arange(len(rings) + 1), vert_off=vert_off, verts=np.concatenate(rings), layers=np.ones(len(rings), int)))
    return nets


def _batch(recipe, R, E, steps, seed=0):
    """The packed batch of a recipe (synthetic.py's builders); its length leaves every scenario running for `steps`."""
    import scenario_gym_amd._lib as L
    from scenario_gym_amd import synthetic

    n = steps + 40
    extent = 8.0 + 2.5 * np.sqrt(E)
    kw = dict(seed=synthetic.SEED + seed)
    if recipe in ("replay", "pid", "vehicle", "pid_sparse"):
        kind = dict(replay=L.KIND_AGENT_REPLAY, pid=L.KIND_AGENT_PID, vehicle=L.KIND_AGENT_VEHICLE, pid_sparse=L.KIND_AGENT_PID)[recipe]
        p = synthetic.make_batch(R, E, n_steps=n, ego_kind=kind, extent=extent, vanish_frac=0.2, **kw)
        if recipe == "pid_sparse":  # a PID ego in every fourth scenario: at most SG_TAB_LANES controlled lanes per wavefront at G = 4
            ego = np.arange(R) * E
            p.kind[ego[np.arange(R) % 4 != 0]] = L.KIND_AGENT_REPLAY
        return p
    side = 4.0 + 1.5 * np.sqrt(E)
    if recipe == "crowd":
        return synthetic.make_crowd(R, E, n_steps=n, side=side, **kw)
    if recipe == "mixed":  # a PID car as the ego of a social-force crowd
        return synthetic.make_crowd_with_car(R, E, n_steps=n, side=side, **kw)
    raise ValueError(recipe)


MODELS = [dict(), dict(relaxation_time=0.8, ped_repulse_V=2.5, ped_repulse_sigma=0.6, sight_angle=160, max_speed_factor=1.1)]


def _stage_inputs(st):
    """(packed, networks, net_of, model_of, actions) of a row / stage."""
    R, E, T = st["R"], st["E"], st["T"]
    from scenario_gym_amd import synthetic

    packed = _batch(st["recipe"], R, E, T, st.get("seed", 0))
    nets = net_of = None
    if st["road"]:
        nets = _nets(11 + st.get("seed", 0))
        net_of = np.random.default_rng(R + E).integers(-1, len(nets), R).astype(np.int32)
        net_of[0] = 0
    model_of = np.random.default_rng(E).integers(0, len(MODELS), R * E).astype(np.int32) if st.get("models") else None
    acts = synthetic.make_actions(T, R, seed=synthetic.SEED + st.get("seed", 0))
    return packed, nets, net_of, model_of, acts


def _new_engine(sga, st, terminal):
    return sga.RolloutEngine(st["R"], st["E"], timestep=DT, terminal_conditions=terminal, event_capacity=64)


def _run(eng, st, inputs):
    """One stage on a handle: knobs, upload, road networks, the entry point's calls."""
    packed, nets, net_of, model_of, acts = inputs
    if st["tuning"]:
        eng.set_tuning(**st["tuning"])
    eng.set_slicing(st["slicing"])
    eng.set_rss(st["rss"])
    if model_of is not None:
        eng.set_ped_models(MODELS, model_of)
    eng.upload(packed)
    if nets is not None:
        eng.set_road_networks(nets, net_of)
    T = st["T"]
    if st["entry"] == "rollout":
        eng.rollout(T)
    elif st["entry"] == "step":
        eng.step(T, acts)
    else:
        for k in range(T):
            eng.tick(acts[k], [0], nw=4, nh=4)
    eng.synchronize()


def _oracle_check(O, eng, st, inputs, terminal_mask, K=3):
    """compare_final (+ the RSS records) on K scenarios spread over the batch: {scenario: [mismatching fields]}."""
    from oracle import check
    from scenario_gym_amd.packing import unpack_scenario

    packed, nets, net_of, model_of, acts = inputs
    E, T = packed.n_entities, st["T"]
    state = eng.state()
    rows, events = eng.metrics()
    rs = eng.rss() if st["rss"] else None
    mrows = None
    if model_of is not None:
        mrows = np.array([O.ped_model_row("social_force", O.social_force_params(**m), 0.0, 0.0) for m in MODELS])
    bad = {}
    for r in check.spread(packed.n_scenarios, K):
        s = unpack_scenario(packed, r)
        veh = (np.asarray(s["kind"]) == O.KIND_AGENT_VEHICLE).any()
        if st["entry"] == "rollout":  # sg_rollout feeds external-action slots (0, 0)
            actions, force = (np.zeros((T, 2)) if veh else None), False
        else:
            actions, force = (acts[:, r] if veh else None), True
        o = O.rollout(s["knot_off"], s["knots"], s["bbox"], s["etype"], s["kind"], s["ego"], s["t0"], s["length"], DT,
                      terminal_mask=terminal_mask, ctrl=s["ctrl"], actions=actions, max_steps=T, force_steps=force, record=True,
                      event_cap=64, route_off=s.get("route_off"), routes=s.get("routes"),
                      road=None if nets is None or net_of[r] < 0 else nets[net_of[r]],
                      models=mrows, model_of=None if model_of is None else model_of[r * E:(r + 1) * E])
        b = check.compare_final(state, rows, events, r, o, E, event_cap=64, kind=packed.kind[r * E:(r + 1) * E])
        if rs is not None:
            q = O.rss_rollout(o, s["bbox"], s["ego"])
            if bool(rs[0][r]) != bool(q["safe_longitudinal"]) or bool(rs[1][r]) != bool(q["safe_lateral"]):
                b.append("rss_flags")
            if not np.array_equal(rs[2][r, :E], q["code"][-1]):
                b.append("rss_codes")
            if not check._bits(rs[3][r, :E], q["safe"][-1]):
                b.append("rss_safe_distances")
        if b:
            bad[r] = b
    return bad


def _terminal(st):
    return ["max_length", "ego_off_road"] if st["road"] else ["max_length"]


@pytest.mark.gpu
@pytest.mark.parametrize("row", VARIANTS, ids=[r["id"] for r in VARIANTS])
def test_variant_matches_oracle(sga, oracle, monkeypatch, row):
    """The row's batch through its entry point: the dispatcher names the row's family, and the results equal the oracle's."""
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    term = _terminal(row)
    inputs = _stage_inputs(row)
    eng = _new_engine(sga, row, term)
    try:
        _run(eng, row, inputs)
        assert eng.last_kernel() == row["expect"]
        bad = _oracle_check(oracle, eng, row, inputs, sga.engine.terminal_mask(term))
        assert not bad, bad
        if row["rss"] and row["E"] <= 512:
            assert (eng.rss()[2] >= 0).any()  # (the callback did run)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ reused handles
def _snapshot(eng, rss, kind, E):
    import scenario_gym_amd._lib as L

    st = eng.state()
    is_ped = np.asarray(kind).reshape(eng.R, E) == L.KIND_AGENT_PEDESTRIAN
    snap = {k: st[k] for k in ("poses", "vels", "present", "dists", "coll", "t", "prev_t", "done", "n_steps", "noise_pos")}
    snap["ctrl_state(not ped)"] = np.where(is_ped[..., None], 0.0, st["ctrl_state"])
    snap["force(ped)"] = np.where(is_ped[..., None], st["force"], 0.0)
    rows, ev = eng.metrics()
    for k in ("ego_avg_speed", "ego_max_speed", "ego_distance_travelled", "final_t", "n_steps", "done", "n_collisions"):
        snap["metric " + k] = rows[k]
    for k in ("t", "scenario", "other", "type"):
        snap["event " + k] = ev[k]
    if rss:
        for k, v in zip(("rss safe_longitudinal", "rss safe_lateral", "rss codes", "rss safe distances"), eng.rss()):
            snap[k] = v
    return snap


def _stage(recipe, E, R, entry, T, rss=False, road=False, tuning=None, seed=0):
    return dict(recipe=recipe, E=E, R=R, entry=entry, T=T, rss=rss, road=road, tuning=NO_TAB if tuning is None else tuning,
                slicing=False, seed=seed, env={})


REUSE = {
    # 257..512 entities: the fused rollout_kernel_rss<64, 8> fills the line-test queue of the handle (dense traffic around the
    # ego), then pedestrians with RSS tick by tick (no fused variant: rss_kernel behind the step), then vehicles again
    "wv8_rss_queue": (["max_length"], [
        _stage("pid", 300, 3, "rollout", 60, rss=True),
        _stage("mixed", 300, 3, "tick", 24, rss=True, seed=1),
        _stage("vehicle", 300, 3, "tick", 16, rss=True, seed=2),
    ]),
    # ... and under ego_off_road, a condition of the handle (sg_create): at 257..512 entities every RSS step of such a handle
    # runs unfused, rollout, pedestrians and vehicles with road networks alike
    "wv8_rss_off_road": (["max_length", "ego_off_road"], [
        _stage("pid", 300, 3, "rollout", 30, rss=True, road=True),
        _stage("mixed", 300, 3, "tick", 12, rss=True, road=True, seed=1),
        _stage("vehicle", 300, 3, "tick", 12, rss=True, road=True, seed=2),
    ]),
    # up to 8 entities: the persistent launch, pedestrians (tile promoted to 16 lanes), the persistent launch again
    "narrow_tiles": (["max_length"], [
        _stage("pid_sparse", 6, 24, "rollout", 40, tuning=TAB),
        _stage("mixed", 6, 24, "rollout", 20, seed=1),
        _stage("pid_sparse", 6, 24, "rollout", 40, tuning=TAB, seed=2),
        _stage("pid_sparse", 6, 24, "step", 40, tuning=TAB, seed=3),
    ]),
    # road networks and RSS switched between stages: nothing of a stage leaks into the next
    "roads_and_rss": (["max_length", "ego_off_road"], [
        _stage("pid", 20, 12, "rollout", 30, rss=True, road=True),
        _stage("pid", 20, 12, "rollout", 30, seed=1),
        _stage("vehicle", 20, 12, "step", 20, rss=True, road=True, seed=2),
        _stage("vehicle", 20, 12, "tick", 10, rss=True, seed=3),
        _stage("mixed", 20, 12, "tick", 10, road=True, seed=4),
    ]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REUSE))
def test_reused_handle_equals_fresh_handle(sga, oracle, name):
    """One handle through a sequence of uploads that change the kernel variant: after every stage its state, metric rows,
    events and RSS records are the bits of a fresh handle running the same stage, and equal the oracle on a few scenarios."""
    term, stages = REUSE[name]
    mask = sga.engine.terminal_mask(term)
    eng = _new_engine(sga, stages[0], term)
    try:
        for i, st in enumerate(stages):
            inputs = _stage_inputs(st)
            _run(eng, st, inputs)
            fresh = _new_engine(sga, st, term)
            try:
                _run(fresh, st, inputs)
                a = _snapshot(eng, st["rss"], inputs[0].kind, st["E"])
                b = _snapshot(fresh, st["rss"], inputs[0].kind, st["E"])
                names = (eng.last_kernel(), fresh.last_kernel())
            finally:
                fresh.close()
            diff = [k for k in a if not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"))]
            assert not diff, f"stage {i} ({st['recipe']} {st['entry']}, kernels {names}): reused handle != fresh handle in {diff}"
            bad = _oracle_check(oracle, eng, st, inputs, mask)
            assert not bad, f"stage {i} ({st['recipe']} {st['entry']}): {bad}"
    finally:
        eng.close()
