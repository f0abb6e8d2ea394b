"""Kernel time of the lane-frame vector observation (sg_lane_observation, device outputs) beside the map raster of the same
tick (sg_raster_map_device: entity + driveable_surface, 128 x 128, the observation of VectorScenarioEnv), for the egos of 4096
scenarios that roam the largest committed network (the 6-lane intersection: 132 lanes, 11,040 centre points).  HIP events on
the handle's stream, both warm, interleaved call by call, median of 20.
    python tools/lane_obs_time.py [k] [n_ahead] [output.json]
Writes profiles/lane_observation_time.json."""
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

K = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N_AHEAD = int(sys.argv[2]) if len(sys.argv) > 2 else 8
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "lane_observation_time.json")
SPACING, RADIUS = 2.0, 30.0
R, E, PX = 4096, 16, 128
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


def main():
    global stream
    rn = network()
    v = rn.polygon_arrays()["verts"]
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=float((v.max(0) - v.min(0)).min()) / 2, vanish_frac=0.3, seed=5)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], np.zeros(R, np.int32))
    eng.set_lanes([rn.lane_arrays()])
    eng.step(5)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    feat = torch.empty((R, K, 6 + 2 * N_AHEAD), dtype=torch.float64, device="cuda:0")
    lanes = torch.empty((R, K), dtype=torch.int32, device="cuda:0")
    count = torch.empty((R,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    layers = np.array([0, LAYER_DRIVEABLE], np.int32)
    d_map = C.c_void_p()
    lane_call = lambda: lib.sg_lane_observation(h, K, N_AHEAD, SPACING, RADIUS, feat.data_ptr(), lanes.data_ptr(), count.data_ptr(), 1)  # noqa: E731
    map_call = lambda: lib.sg_raster_map_device(h, 30.0, 30.0, PX, PX, 2, layers.ctypes.data, C.byref(d_map))  # noqa: E731
    assert lane_call() == 0 and map_call() == 0
    with torch.cuda.stream(stream):
        t_lane, t_map = series([lane_call, map_call])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    a = rn.lane_arrays()
    res = dict(tool="tools/lane_obs_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), shape=[R, E], observers=R,
               network=NETWORK, lanes=len(a["pt_off"]) - 1, centre_points=len(a["pts"]), k=K, n_ahead=N_AHEAD, spacing=SPACING, radius=RADIUS,
               lane_observation=summary(t_lane), map_raster_2x128x128=summary(t_map),
               map_over_lane=float(np.median(t_map) / np.median(t_lane)),
               mean_count=float(count.float().mean()), mean_rows=float((lanes >= 0).float().sum(dim=1).mean()))
    print(f"{R} egos on {NETWORK} ({res['lanes']} lanes, {res['centre_points']} points), k = {K}, n_ahead = {N_AHEAD}, radius {RADIUS}: "
          f"lane_observation_kernel median {res['lane_observation']['median_us']:.0f} us (min {res['lane_observation']['min_us']:.0f}, "
          f"max {res['lane_observation']['max_us']:.0f}); map raster 2 x {PX} x {PX} median {res['map_raster_2x128x128']['median_us']:.0f} us "
          f"(min {res['map_raster_2x128x128']['min_us']:.0f}, max {res['map_raster_2x128x128']['max_us']:.0f}); map / lane "
          f"{res['map_over_lane']:.1f}; mean count {res['mean_count']:.1f}, mean rows {res['mean_rows']:.1f}")
    eng.close()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
