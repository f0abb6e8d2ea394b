"""Kernel time of the route and recorded-track observation (sg_route_observation / sg_route_observation_observers, device outputs)
for the egos of 4096 scenarios and for an observer list of all their entities, every entity with its own recording as its route,
beside sg_lane_observation_observers for the same observer list on the largest committed network (the 6-lane intersection: 132
lanes, 11,040 centre points) for scale.  HIP events on the handle's stream, all warm, interleaved call by call, median of 20.
    python tools/route_obs_time.py [n_ahead] [output.json]
Writes profiles/route_obs_time.json."""
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

N_AHEAD = int(sys.argv[1]) if len(sys.argv) > 1 else 8
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "route_obs_time.json")
SPACING = 2.0
R, E, N_KNOTS = 4096, 16, 16
LANE_K, LANE_RADIUS = 3, 30.0
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
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=N_KNOTS, extent=float((v.max(0) - v.min(0)).min()) / 2, vanish_frac=0.3, seed=5)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], np.zeros(R, np.int32))
    eng.set_lanes([rn.lane_arrays()])
    scen, slot = np.repeat(np.arange(R, dtype=np.int32), E), np.tile(np.arange(E, dtype=np.int32), R)
    off = np.asarray(packed.knot_off, np.int64)
    eng.set_routes(scen, slot, [packed.knots[off[i]:off[i + 1], 1:3] for i in range(R * E)])
    eng.set_observers(scen, slot)
    eng.step(5)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    n = R * E
    feat = torch.empty((n, L.RT_NFEAT + 2 * N_AHEAD), dtype=torch.float64, device="cuda:0")
    info = torch.empty((n, L.RT_NINFO), dtype=torch.int32, device="cuda:0")
    lfeat = torch.empty((n, LANE_K, 6 + 2 * N_AHEAD), dtype=torch.float64, device="cuda:0")
    lanes = torch.empty((n, LANE_K), dtype=torch.int32, device="cuda:0")
    count = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ego_call = lambda: lib.sg_route_observation(h, N_AHEAD, SPACING, feat.data_ptr(), info.data_ptr(), 1)  # noqa: E731
    all_call = lambda: lib.sg_route_observation_observers(h, N_AHEAD, SPACING, feat.data_ptr(), info.data_ptr(), 1)  # noqa: E731
    lane_call = lambda: lib.sg_lane_observation_observers(h, LANE_K, N_AHEAD, SPACING, LANE_RADIUS, lfeat.data_ptr(), lanes.data_ptr(), count.data_ptr(), 1)  # noqa: E731
    assert ego_call() == 0 and all_call() == 0 and lane_call() == 0
    with torch.cuda.stream(stream):
        t_ego, t_all, t_lane = series([ego_call, all_call, lane_call])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    on_route = float((info[:, 0] >= 0).float().mean())
    res = dict(tool="tools/route_obs_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), shape=[R, E], n_ahead=N_AHEAD,
               spacing=SPACING, route_points=N_KNOTS, routes=n, route_observation_egos=dict(observers=R, **summary(t_ego)),
               route_observation_all_entities=dict(observers=n, **summary(t_all)),
               lane_observation_all_entities=dict(observers=n, network=NETWORK, k=LANE_K, radius=LANE_RADIUS, **summary(t_lane)),
               lane_over_route=float(np.median(t_lane) / np.median(t_all)), observers_on_a_route=on_route)
    print(f"{R} x {E}, routes of {N_KNOTS} points, n_ahead = {N_AHEAD}: route_observation_kernel {R} egos median "
          f"{res['route_observation_egos']['median_us']:.0f} us, {n} observers median {res['route_observation_all_entities']['median_us']:.0f} us; "
          f"lane_observation_kernel for the same {n} observers (k = {LANE_K}) median {res['lane_observation_all_entities']['median_us']:.0f} us; "
          f"{100 * on_route:.0f} % of the observers on a route")
    eng.close()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
