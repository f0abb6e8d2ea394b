"""Kernel time of the range scan (sg_range_scan, device outputs) beside the two observations a policy would take in its place:
the map raster of the same tick (sg_raster_map_device: entity + driveable_surface, 128 x 128, the observation of
VectorScenarioEnv) and the nearest-entity rows (sg_nearest_entities, k = 8).  HIP events on the handle's stream, all warm,
interleaved call by call, median / min / max of 20.
    python tools/range_scan_time.py [output.json]
1. 4096 x 64 on the 6-lane intersection, the ego of every scenario: 64 and 256 beams to 100 m, 64 beams to 30 m.
2. 4096 x 64 packed into a 40 m yard, where most beams end on a box: 64 and 256 beams to 100 m.
3. 256 x 1024 (the wide path of the rollout) in a 160 m yard, the ego of every scenario: 64 beams to 100 m.
Writes profiles/range_scan_time.json."""
import ctypes as C
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
from scenario_gym_amd.road_network import LAYER_DRIVEABLE, RoadNetwork

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "range_scan_time.json")
PX, K, RADIUS = 128, 8, 30.0
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


def scan(lib, h, R, n_rays, max_range):
    """(the call, its output tensors) of one scan configuration with device outputs."""
    feat = torch.empty((R, n_rays, 2), dtype=torch.float64, device="cuda:0")
    slots = torch.empty((R, n_rays), dtype=torch.int32, device="cuda:0")
    hits = torch.empty((R,), dtype=torch.int32, device="cuda:0")
    call = lambda: lib.sg_range_scan(h, n_rays, -np.pi, 2.0 * np.pi / n_rays, max_range, feat.data_ptr(), slots.data_ptr(), hits.data_ptr(), 1)  # noqa: E731
    return call, (feat, slots, hits)


def told(name, t, outs, n_rays):
    hits = outs[2].float()
    d = dict(summary(t), mean_hits=float(hits.mean()), hit_fraction=float(hits.mean() / n_rays))
    print(f"  {name}: median {d['median_us']:.0f} us (min {d['min_us']:.0f}, max {d['max_us']:.0f}), {d['hit_fraction']:.0%} of the beams hit")
    return d


def narrow():
    global stream
    R, E = 4096, 64
    rn = network()
    v = rn.polygon_arrays()["verts"]
    extent = float((v.max(0) - v.min(0)).min()) / 2
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=extent, vanish_frac=0.3, seed=5)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], np.zeros(R, np.int32))
    eng.step(5)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    s64, o64 = scan(lib, h, R, 64, 100.0)
    s256, o256 = scan(lib, h, R, 256, 100.0)
    s30, o30 = scan(lib, h, R, 64, 30.0)
    n_feat = torch.empty((R, K, 8), dtype=torch.float64, device="cuda:0")
    n_slots = torch.empty((R, K), dtype=torch.int32, device="cuda:0")
    n_count = torch.empty((R,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    layers = np.array([0, LAYER_DRIVEABLE], np.int32)
    d_map = C.c_void_p()
    near_call = lambda: lib.sg_nearest_entities(h, K, RADIUS, n_feat.data_ptr(), n_slots.data_ptr(), n_count.data_ptr(), 1)  # noqa: E731
    map_call = lambda: lib.sg_raster_map_device(h, 30.0, 30.0, PX, PX, 2, layers.ctypes.data, C.byref(d_map))  # noqa: E731
    calls = [s64, s256, s30, near_call, map_call]
    assert all(c() == 0 for c in calls)
    with torch.cuda.stream(stream):
        t64, t256, t30, t_near, t_map = series(calls)
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    print(f"{R} x {E} on {NETWORK} (extent {extent:.0f} m), the egos:")
    res = dict(shape=[R, E], observers=R, network=NETWORK, extent=extent,
               scan_64_beams_100m=told("64 beams to 100 m", t64, o64, 64), scan_256_beams_100m=told("256 beams to 100 m", t256, o256, 256),
               scan_64_beams_30m=told("64 beams to 30 m", t30, o30, 64), nearest_k8_radius30=summary(t_near), map_raster_2x128x128=summary(t_map))
    res["map_over_scan_64"] = float(np.median(t_map) / np.median(t64))
    print(f"  sg_nearest_entities k = {K}, radius {RADIUS}: median {res['nearest_k8_radius30']['median_us']:.0f} us; map raster 2 x {PX} x {PX}: "
          f"median {res['map_raster_2x128x128']['median_us']:.0f} us (min {res['map_raster_2x128x128']['min_us']:.0f}, "
          f"max {res['map_raster_2x128x128']['max_us']:.0f}); map / 64-beam scan {res['map_over_scan_64']:.1f}")
    eng.close()
    return res


def yard(R, E, extent, rays, steps):
    """The egos of R x E scenarios in a square yard without a network: one scan per beam count, to 100 m."""
    global stream
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=extent, vanish_frac=0.3, seed=6)
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.step(steps)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    scans = [scan(lib, h, R, n, 100.0) for n in rays]
    torch.cuda.synchronize()
    assert all(c() == 0 for c, _ in scans)
    with torch.cuda.stream(stream):
        times = series([c for c, _ in scans])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    print(f"{R} x {E} (extent {extent:.0f} m), the egos:")
    res = dict(shape=[R, E], observers=R, extent=extent)
    for n, t, (_, outs) in zip(rays, times, scans):
        res[f"scan_{n}_beams_100m"] = told(f"{n} beams to 100 m", t, outs, n)
    eng.close()
    return res


if __name__ == "__main__":
    out = dict(tool="tools/range_scan_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), egos_4096x64=narrow(),
               egos_4096x64_dense=yard(4096, 64, 40.0, (64, 256), 5), egos_256x1024=yard(256, 1024, 160.0, (64,), 2))
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
