"""Kernel time of the observer-list observations (sg_raster_map_observers, sg_future_collision_observers; device outputs) on
4096 x 64 entities spread over one road network: HIP events on the handle's stream, warm, median of 20.
    python tools/observers_time.py [R] [E]
1. The ego list -- observer (r, ego of r) for every scenario -- against sg_raster_map_device, the existing ego call, on the
   same handle, interleaved call by call: layers entity + driveable_surface, 20 x 20.  The ratio of the medians is printed beside
   the run-to-run spread of the ego call over its 20 repetitions.
2. Every slot an observer (R * E observers): us and observers/s of both calls, and the map call's output bytes over the HBM
   write rate measured in the same process (a hipMemsetAsync of the same buffer): what bounds it.
The networks are those of tests/golden/roads.npz used by tools/road_info_time.py (the 6-lane intersection and Greenwich_002)."""
import ctypes
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
from scenario_gym_amd import synthetic

R = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
E = int(sys.argv[2]) if len(sys.argv) > 2 else 64
g = np.load(os.path.join("tests", "golden", "roads.npz"))
W, H, NW, NH = 20.0, 20.0, 20, 20
LAY = np.ascontiguousarray([0, 1], np.int32)
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


def stats(x):
    return f"median {np.median(x):.0f} us (min {x.min():.0f}, max {x.max():.0f})"


for net in ("dRisk Unity 6-lane Intersection", "Greenwich_Road_Network_002"):
    a = {k: g[f"net/{net}/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")}
    lo, hi = a["verts"].min(0), a["verts"].max(0)
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=8, static_frac=1.0, vanish_frac=0.0, extent=1.0)
    rng = np.random.default_rng(3)
    packed.knots[:, 1:3] = rng.uniform(lo, hi, (len(packed.knots), 2))  # every entity stands somewhere on the network's extent
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([a], np.zeros(R, np.int32))
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    plane = len(LAY) * NH * NW
    # ---- 1. the ego list against the ego call
    eng.set_observers(np.arange(R), packed.ego)
    out = torch.empty((R, len(LAY), NH, NW), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptr = ctypes.c_void_p()
    ego_call = lambda: lib.sg_raster_map_device(h, W, H, NW, NH, len(LAY), LAY.ctypes.data, ctypes.byref(ptr))  # noqa: E731
    obs_call = lambda: lib.sg_raster_map_observers(h, W, H, NW, NH, len(LAY), LAY.ctypes.data, out.data_ptr(), 1)  # noqa: E731
    t_ego, t_obs = series([ego_call, obs_call])
    lib.sg_synchronize(h)
    same = bool(np.array_equal(out.cpu().numpy(), eng.raster_map(LAY, W, H, NW, NH).astype(np.uint8)))
    spread = (t_ego.max() - t_ego.min()) / np.median(t_ego)
    print(f"{net}: ego list, {R} observers, entity + driveable_surface, {NW} x {NH}: sg_raster_map_observers {stats(t_obs)}; "
          f"sg_raster_map_device {stats(t_ego)}; ratio of medians {np.median(t_obs) / np.median(t_ego):.3f}, spread of the ego call "
          f"(max - min) / median = {spread:.3f}; bytes equal: {same}")
    # ---- 2. every slot an observer
    n = R * E
    eng.set_observers(np.repeat(np.arange(R), E), np.tile(np.arange(E), R))
    out = torch.empty((n, len(LAY), NH, NW), dtype=torch.uint8, device="cuda:0")
    fut = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    all_map = lambda: lib.sg_raster_map_observers(h, W, H, NW, NH, len(LAY), LAY.ctypes.data, out.data_ptr(), 1)  # noqa: E731
    all_fut = lambda: lib.sg_future_collision_observers(h, 5.0, 10, fut.data_ptr(), 1)  # noqa: E731
    with torch.cuda.stream(stream):
        fill = lambda: out.zero_()  # noqa: E731  (the write rate of HBM on this buffer)
        t_map, t_fut, t_fill = series([all_map, all_fut, fill])
    all_map()  # (the fill was the last to write the buffer)
    lib.sg_synchronize(h)
    mb = n * plane / 1e6
    rate = mb / np.median(t_fill) * 1e6 / 1e6  # TB/s
    print(f"{net}: every slot, {n} observers ({mb:.0f} MB of maps): sg_raster_map_observers {stats(t_map)} = "
          f"{n / np.median(t_map):.1f} M observers/s; output-bandwidth floor {np.median(t_fill):.0f} us (fill of the same buffer at "
          f"{rate:.2f} TB/s) = {100 * np.median(t_fill) / np.median(t_map):.0f} % of the call; sg_future_collision_observers "
          f"(horizon 5.0, 10 samples) {stats(t_fut)} = {n / np.median(t_fut):.1f} M observers/s; "
          f"maps set {out.float().mean().item():.4f}, flags set {fut.float().mean().item():.4f}")
    eng.close()
