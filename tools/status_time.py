"""Kernel time of the entity status (sg_entity_status_observers, device outputs) beside what a caller composes today for a part
of it on the same handle: sg_road_info with device outputs (the layers under every entity slot of the batch) plus
sg_nearest_entities_observers at k = 1 (the nearest reference point, not the nearest box).  HIP events on the handle's stream,
all warm, interleaved call by call, median / min / max of 20.
    python tools/status_time.py [output.json]
1. 4096 x 64 and 1024 x 256 on the 6-lane intersection: the ego of every scenario as the observers, then 8 observers per
   scenario (slots 0..7).
2. The driver tick of 4096 x 64 with 8 drivers per scenario: sg_step_drivers alone and followed by the status of the drivers,
   which is what VectorScenarioEnv(drivers=..., driver_status=True) adds to a tick.
Writes profiles/status_time.json."""
import json
import lzma
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic
from scenario_gym_amd.road_network import RoadNetwork

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "status_time.json")
NETWORK = "dRisk Unity 6-lane Intersection"
stream = None


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def series(fns, n=20, warm=3):
    """The functions called in turn, n rounds after `warm` untimed ones: one list of us per function."""
    for _ in range(warm):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            out[k].append(timed(fn))
    return [np.array(o) for o in out]


def summary(x):
    return dict(median_us=float(np.median(x)), min_us=float(x.min()), max_us=float(x.max()), repeats=len(x))


def network():
    with np.load(os.path.join("tests", "golden", "inputs_roads_2.npz")) as g:
        return RoadNetwork.create_from_dict(json.loads(lzma.decompress(g[f"Road_Networks/{NETWORK}.json"].tobytes())), name=NETWORK)


def engine(R, E, rn, drivers=0):
    v = rn.polygon_arrays()["verts"]
    extent = float((v.max(0) - v.min(0)).min()) / 2
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=extent, vanish_frac=0.3, seed=5)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    if drivers:
        kinds = packed.kind.reshape(R, E).copy()
        kinds[:, :drivers] = L.KIND_AGENT_EXTERNAL
        packed.kind = kinds.ravel()
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], np.zeros(R, np.int32))
    return eng, extent


def buffers(n, R, E):
    dev = "cuda:0"
    return dict(flags=torch.empty((n,), dtype=torch.int32, device=dev), info=torch.empty((n, L.ST_NINFO), dtype=torch.int32, device=dev),
                feat=torch.empty((n, L.ST_NFEAT), dtype=torch.float64, device=dev),
                count=torch.empty((R, E), dtype=torch.int32, device=dev), layers=torch.empty((R, E), dtype=torch.int32, device=dev),
                n_feat=torch.empty((n, 1, 8), dtype=torch.float64, device=dev), n_slots=torch.empty((n, 1), dtype=torch.int32, device=dev),
                n_count=torch.empty((n,), dtype=torch.int32, device=dev))


def observers(eng, R, E, per_scenario, name):
    """The status of per_scenario observers per scenario (slots 0 .. per_scenario - 1) beside road_info + nearest k = 1."""
    global stream
    lib, h = eng.lib, eng.h
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(per_scenario), R)
    eng.set_observers(scen, slot)
    n = len(scen)
    b = buffers(n, R, E)
    torch.cuda.synchronize()
    status = lambda: lib.sg_entity_status_observers(h, b["flags"].data_ptr(), b["info"].data_ptr(), b["feat"].data_ptr(), 1)  # noqa: E731
    road = lambda: lib.sg_road_info(h, 0, b["count"].data_ptr(), None, b["layers"].data_ptr(), 1)  # noqa: E731
    near = lambda: lib.sg_nearest_entities_observers(h, 1, float("inf"), b["n_feat"].data_ptr(), b["n_slots"].data_ptr(), b["n_count"].data_ptr(), 1)  # noqa: E731
    calls = [status, road, near]
    assert all(c() == 0 for c in calls)
    with torch.cuda.stream(stream):
        t_status, t_road, t_near = series(calls)
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    flags, feat = b["flags"].cpu().numpy().view(np.uint32), b["feat"].cpu().numpy()
    here = (flags & L.ST_PRESENT) != 0
    d = dict(observers=n, entity_status=summary(t_status), road_info=summary(t_road), nearest_k1=summary(t_near),
             composed_median_us=float(np.median(t_road) + np.median(t_near)),
             present=float(here.mean()), off_road=float(((flags & L.ST_OFF_ROAD) != 0)[here].mean()),
             colliding=float(((flags & L.ST_COLLISION) != 0)[here].mean()), median_clearance=float(np.median(feat[here, 2])))
    print(f"  {name} ({n} observers): sg_entity_status_observers median {d['entity_status']['median_us']:.0f} us (min {d['entity_status']['min_us']:.0f}, "
          f"max {d['entity_status']['max_us']:.0f}); sg_road_info {d['road_info']['median_us']:.0f} us + sg_nearest_entities_observers k = 1 "
          f"{d['nearest_k1']['median_us']:.0f} us = {d['composed_median_us']:.0f} us; {d['off_road']:.0%} off the road, {d['colliding']:.0%} colliding, "
          f"median clearance {d['median_clearance']:.2f} m")
    return d


def batch(R, E, rn):
    global stream
    eng, extent = engine(R, E, rn)
    eng.step(5)
    stream = torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    print(f"{R} x {E} on {NETWORK} (extent {extent:.0f} m):")
    res = dict(shape=[R, E], network=NETWORK, extent=extent, egos=observers(eng, R, E, 1, "the egos"),
               eight_per_scenario=observers(eng, R, E, 8, "8 observers per scenario"))
    eng.close()
    return res


def driver_tick(R, E, rn, per_scenario=8):
    global stream
    eng, _ = engine(R, E, rn, drivers=per_scenario)
    lib, h = eng.lib, eng.h
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(per_scenario), R)
    eng.set_drivers(scen, slot)
    eng.set_observers(scen, slot)
    n = len(scen)
    b = buffers(n, R, E)
    rng = np.random.default_rng(3)
    acts = torch.as_tensor(np.stack([rng.uniform(-2, 2, n), rng.uniform(-0.3, 0.3, n)], -1), device="cuda:0").contiguous()
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    step = lambda: lib.sg_step_drivers(h, 1, acts.data_ptr(), 1)  # noqa: E731

    def both():
        rc = lib.sg_step_drivers(h, 1, acts.data_ptr(), 1)
        return rc or lib.sg_entity_status_observers(h, b["flags"].data_ptr(), b["info"].data_ptr(), b["feat"].data_ptr(), 1)

    assert step() == 0 and both() == 0
    with torch.cuda.stream(stream):
        t_step, t_both = series([step, both])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    d = dict(shape=[R, E], drivers=n, step_drivers=summary(t_step), step_drivers_and_status=summary(t_both),
             added_median_us=float(np.median(t_both) - np.median(t_step)))
    print(f"{R} x {E}, {n} drivers: sg_step_drivers median {d['step_drivers']['median_us']:.0f} us; with the status of the drivers behind it "
          f"{d['step_drivers_and_status']['median_us']:.0f} us (+{d['added_median_us']:.0f} us)")
    eng.close()
    return d


if __name__ == "__main__":
    rn = network()
    out = dict(tool="tools/status_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), batch_4096x64=batch(4096, 64, rn),
               batch_1024x256=batch(1024, 256, rn), driver_tick_4096x64=driver_tick(4096, 64, rn))
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
