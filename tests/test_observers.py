"""Map and look-ahead observations for ANY entity of a scenario: RasterizedMapSensor(entity, ...)
(sensor/map.py:136-271) and FutureCollisionDetector(entity, horizon) (sensor/common.py:60-106) for a list of observers --
sg_set_observers, sg_raster_map_observers, sg_future_collision_observers -- against the real reference's answers for non-ego
entities (tests/golden/observers.npz), against the oracle called with the observer's index as `ego`, and against the ego calls.
The GPU tests go through the C ABI and through the Python layers and read only tests/golden/."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import road_shapes as S
from conftest import load_golden, scenario_arrays
from test_host_api import scenario_from_arrays

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sg_set_observers", "sg_raster_map_observers", "sg_future_collision_observers")
SG_ERR_INVALID, SG_ERR_STATE = -1, -3
ALL_LAYERS = [0, 1, 2, 4, 8, 16, 32, 64]  # entity + the seven surface bits
GRIDS = ((20.0, 20.0, 20, 20), (30.0, 16.0, 31, 17))  # width, height, nw, nh (the second: nw != nh)


@pytest.fixture
def sga():
    import scenario_gym_amd as sga

    return sga


def _codes(g):
    from scenario_gym_amd.road_network import LAYER_CODES

    return [LAYER_CODES[str(x)] for x in g["layers"]]


def _net_arrays(roads, name):
    return {k: roads[f"net/{name}/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")}


def _fixture_scenarios(g, roads):
    """The fixture's scenarios as Scenario objects carrying their road network's polygon arrays (roads.npz)."""
    from scenario_gym_amd.road_network import RoadNetwork

    nets, out = {}, []
    for n in (str(x) for x in g["names"]):
        sc = scenario_from_arrays(scenario_arrays(g, f"{n}/scenario"), g[f"{n}/scenario/refs"])
        name = str(g[f"{n}/network"])
        if name not in nets:
            nets[name] = RoadNetwork(name=name)
            nets[name]._arrays = _net_arrays(roads, name)
        sc.road_network = nets[name]
        out.append(sc)
    return out


def _frames(g, n, i):
    """step -> frame index of observer i's recorded maps."""
    return {int(s): f for f, s in enumerate(g[f"{n}/obs{i}/map_steps"])}


# ---------------------------------------------------------------------------------------------------- CPU
def test_oracle_reproduces_the_fixture(oracle):
    """Every array of observers.npz: oracle.raster_map with the observer's index as `ego` on the recorded poses gives every
    recorded map, cell for cell, and is all zeros where the observer is not in the scene; oracle.future_collision with the
    observer's index and the state's t gives every recorded flag.  No grid point is left out."""
    from scenario_gym_amd.packing import default_kinds

    g, roads = load_golden("observers"), load_golden("roads")
    codes = _codes(g)
    maps = ones = flags = absent = 0
    assert len(g["names"]) >= 4
    for n in (str(x) for x in g["names"]):
        s = scenario_arrays(g, f"{n}/scenario")
        kind = default_kinds(len(s["bbox"]), int(s["ego"]))
        net = oracle.RoadNetworkArrays(_net_arrays(roads, str(g[f"{n}/network"])))
        obs = [int(k) for k in g[f"{n}/observers"]]
        assert len(obs) >= 3 and int(s["ego"]) not in obs
        ts, want = g[f"{n}/t"], g[f"{n}/future"].astype(bool)
        for i, k in enumerate(obs):
            for hi, h in enumerate(g["horizons"]):
                got = np.array([oracle.future_collision(s["knot_off"], s["knots"], s["bbox"], kind, k, t, h) for t in ts])
                assert np.array_equal(got, want[:, i, hi]), (n, k, h)
                flags += int(got.sum())
            at = _frames(g, n, i)
            for f, step in enumerate(g[f"{n}/frame_steps"]):
                poses = g[f"{n}/poses"][f]
                assert (int(step) in at) == (not np.isnan(poses[k, 0]))
                for c, (w, h, m) in enumerate(g["raster_cfg"]):
                    got = oracle.raster_map(poses, s["bbox"], k, net, codes, width=w, height=h, nw=int(m), nh=int(m))
                    if int(step) in at:
                        ref = g[f"{n}/obs{i}/map{c}"][at[int(step)]].astype(bool)
                        assert np.array_equal(got, ref), (n, k, c, int(step), int((got != ref).sum()))
                        maps += 1
                        ones += int(got.sum())
                    else:
                        assert not got.any()
                        absent += 1
    assert maps > 1000 and ones > 500000 and flags > 50 and absent > 0


def test_abi_declares_the_observer_calls():
    """_lib.SYMBOLS, the binding's ABI version and include/sgym.h name the three entry points of ABI 7."""
    import scenario_gym_amd._lib as L

    header = open(os.path.join(ROOT, "include", "sgym.h")).read()
    assert L.ABI_VERSION == 7 and re.search(r"#define SG_ABI_VERSION 7\b", header)
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS
        assert re.search(r"\bint " + name + r"\(sg_handle \*h", header), name


def test_fixture_regenerates_byte_for_byte(tmp_path):
    """make_golden_observers.py, run in a fresh interpreter with a random hash seed against the real reference, writes the
    committed observers.npz again, array by array and byte for byte (skipped where the reference is not installed)."""
    if not os.path.isdir("/root/reference/scenario_gym"):
        pytest.skip("the reference is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regen_golden

    assert regen_golden.GENERATORS["make_golden_observers"] == ["observers"]
    regen_golden.run_generator("make_golden_observers", str(tmp_path))
    ok, n, bad = regen_golden.compare_file("observers", str(tmp_path))
    assert not bad and ok == n > 50, bad[:6]


# ---------------------------------------------------------------------------------------------------- GPU: the C ABI
def _raw(eng, n, layers, grid, device=False):
    """sg_raster_map_observers through ctypes into a sentinel-filled buffer of n observers: (rc, uint8 [n, L, nh, nw])."""
    w, h, nw, nh = grid
    lay = np.ascontiguousarray(layers, np.int32)
    out = np.full((n, len(lay), nh, nw), 0xCC, np.uint8)
    rc = eng.lib.sg_raster_map_observers(eng.h, w, h, nw, nh, len(lay), lay.ctypes.data, out.ctypes.data, 0)
    return rc, out


def _raw_future(eng, n, horizon=5.0, n_samples=10):
    out = np.full(n, 0xCC, np.uint8)
    rc = eng.lib.sg_future_collision_observers(eng.h, horizon, n_samples, out.ctypes.data, 0)
    return rc, out


def _has_no_observers(eng):
    """Both observation calls succeed and write nothing."""
    rc, out = _raw(eng, 4, [0, 1], GRIDS[0])
    rf, fut = _raw_future(eng, 4)
    return rc == 0 and rf == 0 and (out == 0xCC).all() and (fut == 0xCC).all()


def _shape_networks():
    rng = np.random.default_rng(11)
    return [S.lattice(rng, offset=(-20.0, -20.0))[0], S.stars(rng, offset=(-5.0, -5.0))[0]]


def _batch_with_networks(sga, R, E, seed=7, n_steps=100):
    """A seeded synthetic batch (a tenth of the entities static, three tenths spawn late and vanish) roaming 40 m x 40 m, scenario
    r on network r % 2 of tests/road_shapes.py; the last scenario of three or more has none."""
    from scenario_gym_amd import synthetic

    packed = synthetic.make_batch(R, E, n_steps=n_steps, timestep=0.1, n_knots=16, extent=20.0, vanish_frac=0.3, seed=seed)
    nets = _shape_networks()
    net_of = np.arange(R, dtype=np.int32) % 2
    if R >= 3:
        net_of[R - 1] = -1
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks(nets, net_of)
    return eng, packed, nets, net_of


@gpu
def test_device_matches_the_reference_fixture(sga):
    """The fixture's scenarios as ONE ragged batch stepped on the device at dt = 0.1, the observers those the fixture
    recorded (non-ego entities; late spawners, vanishing ones, pedestrians): both look-ahead flags at every state and the
    four-layer maps of both grid configurations at every 4th state equal the reference's; an observer that is not in the scene
    gets all zeros."""
    from scenario_gym_amd.packing import pack_scenarios

    g, roads = load_golden("observers"), load_golden("roads")
    names = [str(x) for x in g["names"]]
    scs = _fixture_scenarios(g, roads)
    packed, _ = pack_scenarios(scs)
    eng = sga.RolloutEngine(packed.n_scenarios, packed.n_entities, timestep=0.1)
    eng.upload(packed)
    index, nets, net_of = {}, [], []
    for sc in scs:
        if id(sc.road_network) not in index:
            index[id(sc.road_network)] = len(nets)
            nets.append(sc.road_network.polygon_arrays())
        net_of.append(index[id(sc.road_network)])
    eng.set_road_networks(nets, net_of)
    obs = [(r, int(k), i) for r, n in enumerate(names) for i, k in enumerate(g[f"{n}/observers"])]
    eng.set_observers([o[0] for o in obs], [o[1] for o in obs])
    codes = _codes(g)
    frames = {(r, i): _frames(g, names[r], i) for r, _, i in obs}
    last = max(len(g[f"{n}/t"]) for n in names) - 1
    maps = absent = flags = 0
    for step in range(last + 1):
        t = eng.state()["t"]
        live = [r for r, n in enumerate(names) if step < len(g[f"{n}/t"])]
        for r in live:
            assert t[r] == g[f"{names[r]}/t"][step], (names[r], step)
        fut = [eng.future_collision_observers(float(h)) for h in g["horizons"]]
        for j, (r, k, i) in enumerate(obs):
            if r in live:
                want = g[f"{names[r]}/future"][step, i].astype(bool)
                assert [bool(f[j]) for f in fut] == list(want), (names[r], k, step)
                flags += int(want.sum())
        if step % 4 == 0:
            for c, (w, h, m) in enumerate(g["raster_cfg"]):
                got = eng.raster_map_observers(codes, w, h, int(m), int(m))
                assert got.shape == (len(obs), len(codes), int(m), int(m))
                for j, (r, k, i) in enumerate(obs):
                    if r not in live:
                        continue
                    f = frames[(r, i)].get(step)
                    if f is None:
                        assert not got[j].any(), (names[r], k, step)
                        absent += 1
                    else:
                        want = g[f"{names[r]}/obs{i}/map{c}"][f].astype(bool)
                        assert np.array_equal(got[j], want), (names[r], k, c, step, int((got[j] != want).sum()))
                        maps += 1
        if step < last:
            eng.step(1)
    eng.close()
    assert maps > 1000 and absent > 0 and flags > 50


@gpu
@pytest.mark.parametrize("E", [5, 64, 200, 512, 700])
def test_device_matches_the_oracle_on_seeded_batches(sga, oracle, E):
    """Every slot of a seeded synthetic batch on tests/road_shapes.py networks is an observer (5, 64, 200, 512 and 700 entity
    slots: tiles of a wavefront, one and several wavefronts per scenario, the multi-kernel step): all eight layers in two grid
    shapes (one with nw != nh) and the look-ahead, after the reset and after some steps, equal the oracle called with the
    observer's index as `ego` -- all bytes."""
    R = 3
    eng, packed, nets, net_of = _batch_with_networks(sga, R, E, seed=7 + E)
    onets = [oracle.RoadNetworkArrays(a) for a in nets]
    scen, slot = np.repeat(np.arange(R), E), np.tile(np.arange(E), R)
    assert (packed.kind != 0).all()  # (synthetic batches have no padding slots)
    eng.set_observers(scen, slot)
    ones = np.zeros(len(ALL_LAYERS), np.int64)
    hits = absent = 0
    for steps in (0, 25):
        eng.step(steps)
        st = eng.state()
        for w, h, nw, nh in GRIDS:
            got = eng.raster_map_observers(ALL_LAYERS, w, h, nw, nh)
            assert got.shape == (R * E, 8, nh, nw)
            for r in range(R):
                net = onets[net_of[r]] if net_of[r] >= 0 else None
                bbox = packed.bbox[r * E:(r + 1) * E]
                for e in range(E):
                    want = oracle.raster_map(st["poses"][r], bbox, e, net, ALL_LAYERS, width=w, height=h, nw=nw, nh=nh)
                    j = r * E + e
                    assert np.array_equal(got[j], want), (r, e, steps, (w, h, nw, nh), int((got[j] != want).sum()))
                    if not st["present"][r, e]:
                        assert not got[j].any()
                        absent += 1
                    ones += want.sum(axis=(1, 2))
        for horizon, n_samples in ((5.0, 10), (2.0, 70)):  # (70 samples: more than one round of the kernel's LDS table)
            fut = eng.future_collision_observers(horizon, n_samples)
            for r in range(R):
                a, b = packed.knot_off[r * E], packed.knot_off[(r + 1) * E]
                off, knots = packed.knot_off[r * E:(r + 1) * E + 1] - a, packed.knots[a:b]
                kind, bbox = packed.kind[r * E:(r + 1) * E], packed.bbox[r * E:(r + 1) * E]
                for e in range(E):
                    want = oracle.future_collision(off, knots, bbox, kind, e, float(st["t"][r]), horizon, n_samples)
                    assert bool(fut[r * E + e]) == want, (r, e, steps, horizon)
                    hits += int(want)
    eng.close()
    assert ones[0] > 0 and (ones[1:] > 0).sum() >= 4 and absent > 0
    assert hits > 0 or E == 5


@gpu
def test_ego_list_equals_the_ego_calls(sga):
    """With the observers (r, ego of r) for every scenario, sg_raster_map_observers equals sg_raster_map and
    sg_future_collision_observers equals sg_future_collision, byte for byte, on a batch that has networks (and one scenario
    without); some egos are not in the scene at some of the states."""
    R, E = 48, 16
    eng, packed, nets, net_of = _batch_with_networks(sga, R, E, seed=3)
    eng.set_observers(np.arange(R), packed.ego)
    surface = entity = fut = 0
    for steps in (0, 1, 30, 40, 60):  # (the last: beyond the end of the scenarios)
        eng.step(steps)
        for w, h, nw, nh in GRIDS:
            want = eng.raster_map(ALL_LAYERS, w, h, nw, nh)
            got = eng.raster_map_observers(ALL_LAYERS, w, h, nw, nh)
            assert got.shape == want.shape and np.array_equal(got, want), (steps, int((got != want).sum()))
            entity += int(want[:, 0].sum())
            surface += int(want[:, 1:].sum())
        for horizon, n_samples in ((5.0, 10), (1.0, 10), (3.0, 130)):
            want = eng.future_collision(horizon, n_samples)
            got = eng.future_collision_observers(horizon, n_samples)
            assert np.array_equal(got, want), (steps, horizon)
            fut += int(want.sum())
    eng.close()
    assert entity > 0 and surface > 0 and fut > 0


@gpu
@pytest.mark.parametrize("E", [5, 300, 560])
def test_ego_calls_with_layer_lists_of_any_order_and_length_match_the_oracle(sga, oracle, E):
    """The ego calls on layer lists that only the one-pass raster serves in a single body: sg_raster_map with the entity layer
    not first and twice ([2, 0, 1, 0]) and with nine layers (two launches of at most eight), sg_tick with [2, 0, 1] -- at 5
    entity slots (a tile of less than a wavefront in a 256-thread block), 300 (the 512-thread block) and 560 (tile by tile, the
    multi-kernel step; sg_tick's branch of two launches).  After the reset and after 25 steps every byte equals
    oracle.raster_map on the state's poses; the flags of sg_tick equal sg_terminal_flags of a twin handle stepped by sg_step.
    The ego of the synthetic family (an agent in slot 0) is in the scene throughout, so scenario 1 gets a late spawner as its
    ego: not in the scene at the reset.  Seeds chosen with the oracle on the CPU so that every layer has set bytes."""
    R, (w, h, nw, nh) = 3, GRIDS[1]
    eng, packed, nets, net_of = _batch_with_networks(sga, R, E, seed={5: 5, 300: 1, 560: 1}[E])
    first, n_knots = packed.knots[packed.knot_off[E:2 * E], 0], np.diff(packed.knot_off[E:2 * E + 1])
    packed.ego[1] = np.nonzero((n_knots > 1) & (first > 0.2) & (first <= 2.0))[0][0]
    twin = sga.RolloutEngine(R, E, timestep=0.1)
    for e in (eng, twin):
        e.upload(packed)
        e.set_road_networks(nets, net_of)
    onets = [oracle.RoadNetworkArrays(a) for a in nets]
    ones = dict.fromkeys(ALL_LAYERS, 0)
    absent = 0

    def expected(st, layers):
        want = np.stack([oracle.raster_map(st["poses"][r], packed.bbox[r * E:(r + 1) * E], int(packed.ego[r]),
                                           onets[net_of[r]] if net_of[r] >= 0 else None, layers, width=w, height=h, nw=nw, nh=nh)
                         for r in range(R)])
        for l, code in enumerate(layers):
            ones[code] += int(want[:, l].sum())
        return want

    for advance in (0, 24):  # the states after 0 and 25 steps for sg_raster_map, sg_tick from each of them
        eng.step(advance)
        twin.step(advance)
        st = eng.state()
        assert int(st["n_steps"].max()) == (25 if advance else 0)
        absent += sum(not st["present"][r, packed.ego[r]] for r in range(R))
        for layers in ([2, 0, 1, 0], ALL_LAYERS + [0]):
            got, want = eng.raster_map(layers, w, h, nw, nh), expected(st, layers)
            assert got.shape == want.shape == (R, len(layers), nh, nw)
            assert np.array_equal(got, want), (advance, layers, int((got != want).sum()))
        obs, flags = eng.tick(None, [2, 0, 1], w, h, nw, nh)
        twin.step(1)
        want = expected(eng.state(), [2, 0, 1])
        assert np.array_equal(obs, want), (advance, int((obs != want).sum()))
        assert np.array_equal(flags, twin.terminal_flags()), (advance, flags)
    eng.close()
    twin.close()
    assert all(n > 0 for n in ones.values()), ones
    assert absent > 0


@gpu
def test_device_outputs(sga):
    """Device outputs (torch tensors the kernels write directly) equal the host outputs; a device-output call queued right
    behind sg_step, without a synchronize in between, sees the stepped state."""
    import torch

    R, E = 16, 64
    eng, packed, nets, net_of = _batch_with_networks(sga, R, E, seed=5)
    scen, slot = np.repeat(np.arange(R), 8), np.tile(np.arange(0, E, 8), R)
    eng.set_observers(scen, slot)
    n = len(scen)
    eng.step(10)
    w, h, nw, nh = GRIDS[1]
    host = eng.raster_map_observers(ALL_LAYERS, w, h, nw, nh)
    dev = eng.raster_map_observers(ALL_LAYERS, w, h, nw, nh, torch_out=True)
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == host.shape
    assert np.array_equal(dev.cpu().numpy().astype(bool), host) and host.any()
    hf = eng.future_collision_observers(5.0, 10)
    df = eng.future_collision_observers(5.0, 10, torch_out=True)
    assert df.is_cuda and tuple(df.shape) == (n,) and np.array_equal(df.cpu().numpy().astype(bool), hf)
    # queued behind the step on the handle's stream
    lay = np.ascontiguousarray(ALL_LAYERS, np.int32)
    maps = torch.full((n, 8, nh, nw), 0xCC, dtype=torch.uint8, device="cuda:0")
    flags = torch.full((n,), 0xCC, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.sg_step(eng.h, 15, None, 0) == 0
    assert eng.lib.sg_raster_map_observers(eng.h, w, h, nw, nh, 8, lay.ctypes.data, maps.data_ptr(), 1) == 0
    assert eng.lib.sg_future_collision_observers(eng.h, 5.0, 10, flags.data_ptr(), 1) == 0
    assert eng.lib.sg_synchronize(eng.h) == 0
    after = eng.raster_map_observers(ALL_LAYERS, w, h, nw, nh)
    assert int(eng.state()["n_steps"].max()) == 25
    assert np.array_equal(maps.cpu().numpy().astype(bool), after) and not np.array_equal(after, host)
    assert np.array_equal(flags.cpu().numpy().astype(bool), eng.future_collision_observers(5.0, 10))
    eng.close()


@gpu
def test_lifetime_of_the_observer_list(sga):
    """The list survives sg_reset, sg_step and sg_rollout; duplicates and any order are honoured; n == 0 clears it and
    sg_upload forgets it: the observation calls then succeed and write nothing."""
    R, E = 6, 16
    eng, packed, nets, net_of = _batch_with_networks(sga, R, E, seed=9)
    assert _has_no_observers(eng)
    scen, slot = np.repeat(np.arange(R), E), np.tile(np.arange(E), R)
    eng.set_observers(scen, slot)
    eng.step(12)
    base = eng.raster_map_observers([0, 1, 16], *GRIDS[0])
    base_f = eng.future_collision_observers(5.0, 10)
    assert base.shape[0] == R * E and base.any()
    pick = np.array([95, 3, 3, 40, 0, 95, 17, 64, 3], np.int64)  # any order, with duplicates
    eng.set_observers(scen[pick], slot[pick])
    assert np.array_equal(eng.raster_map_observers([0, 1, 16], *GRIDS[0]), base[pick])
    assert np.array_equal(eng.future_collision_observers(5.0, 10), base_f[pick])
    eng.reset()
    eng.step(12)
    assert np.array_equal(eng.raster_map_observers([0, 1, 16], *GRIDS[0]), base[pick])
    eng.rollout(12)  # reset + 12 steps again
    rc, raw = _raw(eng, len(pick), [0, 1, 16], GRIDS[0])
    assert rc == 0 and np.array_equal(raw.astype(bool), base[pick]) and (raw <= 1).all()
    eng.set_observers([], [])
    assert _has_no_observers(eng)
    eng.set_observers(scen[pick], slot[pick])
    eng.upload(packed)
    assert _has_no_observers(eng)
    eng.close()


@gpu
def test_refusals_are_loud_and_clear_the_list(sga):
    """Every refusal of sg_set_observers: its error code, a message in sg_last_error, and a handle without observers afterwards
    (the rule of the road networks); bad arguments of the two observation calls."""
    from scenario_gym_amd.packing import pack_scenarios

    g, roads = load_golden("observers"), load_golden("roads")
    packed, _ = pack_scenarios(_fixture_scenarios(g, roads))
    R, E = packed.n_scenarios, packed.n_entities
    kind = packed.kind.reshape(R, E)
    assert (kind == 0).any()  # a ragged batch: padding slots of SG_KIND_NONE
    r_pad, e_pad = (int(x[0]) for x in np.nonzero(kind == 0))
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    lib, h = eng.lib, eng.h
    i32 = lambda *v: np.ascontiguousarray(v, np.int32)  # noqa: E731
    one = i32(0)

    def refused(code, n, scen, slot):
        rc = lib.sg_set_observers(h, n, None if scen is None else scen.ctypes.data, None if slot is None else slot.ctypes.data)
        assert rc == code, (rc, code, n)
        assert lib.sg_last_error(h).decode().startswith("sg_set_observers")

    refused(SG_ERR_STATE, 1, one, one)  # before sg_upload
    eng.upload(packed)
    good = (i32(0, 1, 2), i32(1, 1, 1))
    for n, scen, slot in ((-1, one, one), (1, None, one), (1, one, None), (1, i32(-1), one), (1, i32(R), one),
                          (1, one, i32(-1)), (1, one, i32(E)), (2, i32(0, r_pad), i32(0, e_pad)),
                          (2 ** 31, one, one)):  # (more observers than a grid has workgroups: refused before the arrays are read)
        eng.set_observers(*good)
        rc, out = _raw(eng, 3, [0], GRIDS[0])
        assert rc == 0 and (out <= 1).all()
        refused(SG_ERR_INVALID, n, scen, slot)
        assert _has_no_observers(eng)
    eng.set_observers(*good)
    w, hh, nw, nh = GRIDS[0]
    lay = i32(0, 1)
    out = np.zeros((3, 2, nh, nw), np.uint8)
    for args in ((w, hh, nw, nh, 0, lay), (w, hh, nw, nh, 9, lay), (w, hh, 0, nh, 2, lay), (w, hh, nw, 0, 2, lay),
                 (-1.0, hh, nw, nh, 2, lay), (w, float("nan"), nw, nh, 2, lay), (w, hh, nw, nh, 2, i32(0, 3)),
                 (w, hh, nw, nh, 2, i32(0, 256)), (w, hh, nw, nh, 2, None)):
        rc = lib.sg_raster_map_observers(h, *args[:5], None if args[5] is None else args[5].ctypes.data, out.ctypes.data, 0)
        assert rc == SG_ERR_INVALID and lib.sg_last_error(h).decode().startswith("sg_raster_map_observers"), args
    assert lib.sg_raster_map_observers(h, w, hh, nw, nh, 2, lay.ctypes.data, None, 0) == SG_ERR_INVALID
    fut = np.zeros(3, np.uint8)
    for horizon, n_samples in ((-1.0, 10), (float("nan"), 10), (5.0, 0)):
        assert lib.sg_future_collision_observers(h, horizon, n_samples, fut.ctypes.data, 0) == SG_ERR_INVALID
        assert lib.sg_last_error(h).decode().startswith("sg_future_collision_observers")
    assert lib.sg_future_collision_observers(h, 5.0, 10, None, 0) == SG_ERR_INVALID
    rc, out = _raw(eng, 3, [0], GRIDS[0])  # bad arguments of the observation calls leave the list alone
    assert rc == 0 and (out <= 1).all()
    eng.close()
    fresh = sga.RolloutEngine(R, E, timestep=0.1)  # the observation calls before sg_upload
    assert _raw(fresh, 1, [0], GRIDS[0])[0] == SG_ERR_STATE and _raw_future(fresh, 1)[0] == SG_ERR_STATE
    fresh.close()


# ---------------------------------------------------------------------------------------------------- GPU: the Python layers
def _recording_agent(sga, log):
    class Watcher(sga.Agent):
        """A user's agent of a non-ego entity: a Python _step over a CombinedSensor of the map and the look-ahead."""

        def __init__(self, entity, cfg, layers):
            w, h, m = cfg
            sensor = sga.CombinedSensor(entity,
                                        sga.RasterizedMapSensor(entity, layers=layers, width=w, height=h, freq=None, n=int(m), channels_first=True),
                                        sga.FutureCollisionDetector(entity, horizon=5.0))
            super().__init__(entity, sga.ReplayTrajectoryController(entity), sensor)

        def _step(self, observation):
            log.append((self.entity, observation.t, np.array(observation.map), bool(observation.future_collision)))
            return sga.TeleportAction(pose=self.entity.trajectory.position_at_t(observation.next_t))

    return Watcher


@gpu
def test_sensor_classes_reproduce_the_fixture(sga):
    """ScenarioGym, one fixture scenario at a time: RasterizedMapSensor(e) and FutureCollisionDetector(e) of every recorded
    non-ego entity e, stepped by the caller on gym.state, return the reference's maps (both grid configurations, every 4th
    state) and flags (both horizons, every state); State.raster_map / State.future_collision take `entity`.  Then the same
    with one of the entities driven by a user's agent whose CombinedSensor holds both sensors: what the agent saw at every
    tick is the reference's observation of that state."""
    g, roads = load_golden("observers"), load_golden("roads")
    layers = [str(x) for x in g["layers"]]
    names = [str(x) for x in g["names"]]
    maps = flags = seen = 0
    for r, sc in enumerate(_fixture_scenarios(g, roads)):
        n = names[r]
        ts = g[f"{n}/t"]
        obs = [int(k) for k in g[f"{n}/observers"]]
        # ---- sensors stepped by the caller
        gym = sga.ScenarioGym(timestep=0.1)
        gym.set_scenario(sc)
        ents = gym.state.scenario.entities
        rasters = [[sga.RasterizedMapSensor(ents[k], layers=layers, width=w, height=h, freq=None, n=int(m)) for w, h, m in g["raster_cfg"]]
                   for k in obs]
        detectors = [[sga.FutureCollisionDetector(ents[k], horizon=float(h)) for h in g["horizons"]] for k in obs]
        frames = [_frames(g, n, i) for i in range(len(obs))]
        for step in range(len(ts)):
            assert gym.state.t == ts[step]
            for i, k in enumerate(obs):
                got = [d.step(gym.state).future_collision for d in detectors[i]]
                assert got == list(g[f"{n}/future"][step, i].astype(bool)), (n, k, step)
                flags += sum(got)
                if step % 4 == 0:
                    f = frames[i].get(step)
                    assert (f is not None) == (ents[k] in gym.state.poses)
                    for c, rs in enumerate(rasters[i]):
                        m = rs.step(gym.state).map  # [n][n][layer]
                        want = g[f"{n}/obs{i}/map{c}"][f].astype(bool) if f is not None else np.zeros_like(m.transpose(2, 0, 1))
                        assert np.array_equal(m.transpose(2, 0, 1), want), (n, k, c, step)
                        maps += 1
            if step == 8:
                w, h, m = g["raster_cfg"][1]
                a = gym.state.raster_map(layers, w, h, int(m), int(m), entity=ents[obs[0]])
                assert np.array_equal(a, rasters[0][1].step(gym.state).map.transpose(2, 0, 1))
                assert np.array_equal(gym.state.raster_map(layers, w, h, int(m), int(m), entity=sc.ego),
                                      gym.state.raster_map(layers, w, h, int(m), int(m)))
                assert gym.state.future_collision(5.0, entity=ents[obs[0]]) == bool(g[f"{n}/future"][step, 0, 0])
            if step + 1 < len(ts):
                gym.step()
        gym.close()
        # ---- a user's agent of the first recorded entity
        log = []
        Watcher = _recording_agent(sga, log)
        cfg = g["raster_cfg"][0]
        ref = str(g[f"{n}/scenario/refs"][obs[0]])
        gym = sga.ScenarioGym(timestep=0.1)
        gym.set_scenario(sc, create_agent=lambda s, e: Watcher(e, cfg, layers) if e.ref == ref else
                         (sga.ReplayTrajectoryAgent(e) if e.ref == "ego" else None))
        for step in range(len(ts) - 1):
            gym.step()
        gym.close()
        at = {float(t): k for k, t in enumerate(ts)}
        assert len(log) > 10
        for _, t, m, fc in log:
            step = at[t]
            assert fc == bool(g[f"{n}/future"][step, 0, 0]), (n, step)
            if step in frames[0]:
                assert np.array_equal(m, g[f"{n}/obs0/map0"][frames[0][step]].astype(bool)), (n, step)
                seen += 1
    recorded = sum(len(g[f"{n}/frame_steps"]) * len(g[f"{n}/observers"]) * len(g["raster_cfg"]) for n in names)
    assert maps == recorded > 1000 and flags > 50 and seen > 50


@gpu
def test_batched_gym_makes_one_call_per_step_and_configuration(sga):
    """A BatchedScenarioGym of the fixture's scenarios with two user agents of non-ego entities per scenario, all with the same
    sensor configuration: the registry holds every one of them from the start, and a tick costs ONE sg_raster_map_observers
    and ONE sg_future_collision_observers call for the whole batch; what each agent saw is the reference's observation."""
    g, roads = load_golden("observers"), load_golden("roads")
    layers = [str(x) for x in g["layers"]]
    names = [str(x) for x in g["names"]]
    scs = _fixture_scenarios(g, roads)
    log = []
    Watcher = _recording_agent(sga, log)
    cfg = g["raster_cfg"][0]
    watched = {id(sc): [str(g[f"{n}/scenario/refs"][int(k)]) for k in g[f"{n}/observers"][:2]] for sc, n in zip(scs, names)}
    gym = sga.BatchedScenarioGym(timestep=0.1, record=True)  # (the sensors' observations carry State.recorded_poses)
    gym.set_scenarios(scs, create_agent=lambda s, e: Watcher(e, cfg, layers) if e.ref in watched[id(s)] else
                      (sga.ReplayTrajectoryAgent(e) if e.ref == "ego" else None))
    assert sorted(gym._observers) == sorted((r, int(k)) for r, n in enumerate(names) for k in g[f"{n}/observers"][:2])
    calls = {"map": 0, "fut": 0}
    real_map, real_fut = gym.engine.raster_map_observers, gym.engine.future_collision_observers

    def count(key, fn):
        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapped

    gym.engine.raster_map_observers = count("map", real_map)
    gym.engine.future_collision_observers = count("fut", real_fut)
    ticks = 40
    expected = 0
    for tick in range(ticks):
        # a state costs one call of each kind when some watched entity is in the scene (an agent whose entity is not is not
        # stepped); the first state was observed by the agents' reset, before the counters were installed, and is cached
        if tick > 0 and any(a.entity in gym.states[i].poses for i, _, a in gym._host_agents):
            expected += 1
        gym.step()
    assert calls["map"] == calls["fut"] == expected and expected > ticks // 2
    gym.close()
    who = {}
    for r, (sc, n) in enumerate(zip(scs, names)):
        for i, k in enumerate(g[f"{n}/observers"][:2]):
            who[id(sc.entities[int(k)])] = (n, i)
    seen = 0
    for entity, t, m, fc in log:
        n, i = who[id(entity)]
        step = int(np.nonzero(g[f"{n}/t"] == t)[0][0])
        assert fc == bool(g[f"{n}/future"][step, i, 0]), (n, i, step)
        fr = _frames(g, n, i)
        if step in fr:
            assert np.array_equal(m, g[f"{n}/obs{i}/map0"][fr[step]].astype(bool)), (n, i, step)
            seen += 1
    assert seen > 50


@gpu
def test_vector_env_observe_entities(sga):
    """VectorScenarioEnv.set_observers / observe_entities: the maps of engine.raster_map_observers with the environment's
    layers and geometry, host and torch forms, beside an unchanged step / reset."""
    import torch

    g, roads = load_golden("observers"), load_golden("roads")
    scs = _fixture_scenarios(g, roads)
    slots = [[int(k) for k in g[f"{n}/observers"]] for n in (str(x) for x in g["names"])]
    layers = ["entity", "driveable_surface", "lane"]
    for torch_obs in (False, True):
        env = sga.VectorScenarioEnv(scs, timestep=0.1, layers=layers, height=24.0, width=24.0, n=32, auto_reset=False, torch_obs=torch_obs)
        first = env.reset()
        assert env.observe_entities()[0].shape[0] == 0  # no observers yet
        env.set_observers(slots)
        for _ in range(6):
            obs, reward, done, info = env.step(np.zeros((env.n_envs, 2)))
        maps, env_of, slot = env.observe_entities()
        want = env.engine.raster_map_observers([0, 1, 8], 24.0, 24.0, 32, 32)
        if torch_obs:
            assert maps.is_cuda and env_of.is_cuda and slot.is_cuda and maps.dtype == torch.uint8
            maps, env_of, slot = maps.cpu().numpy().astype(bool), env_of.cpu().numpy(), slot.cpu().numpy()
        assert maps.shape == (sum(len(s) for s in slots), 3, 32, 32) and np.array_equal(maps, want) and want.any()
        assert list(env_of) == [i for i, s in enumerate(slots) for _ in s] and list(slot) == [k for s in slots for k in s]
        assert tuple(first.shape) == (env.n_envs, 3, 32, 32)
        env.close()
