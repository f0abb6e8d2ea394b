"""Kernel time of the per-entity road query (sg_road_info, device outputs, cap = 32) on 4096 x 64 entities spread over one road
network, beside one sg_raster_map_device call of the default 20 x 20 x 8 layers on the same batch: HIP events on the handle's
stream, warm, median of 20.    python tools/road_info_time.py [R] [E]
The networks are those of tests/golden/roads.npz (the 6-lane intersection and Greenwich_002)."""
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
stream = None


def median_ms(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


for net in ("dRisk Unity 6-lane Intersection", "Greenwich_Road_Network_002"):
    a = {k: g[f"net/{net}/{k}"] for k in ("ring_off", "vert_off", "verts", "layers")}
    lo, hi = a["verts"].min(0), a["verts"].max(0)
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=8, static_frac=1.0, vanish_frac=0.0, extent=1.0)
    rng = np.random.default_rng(3)
    packed.knots[:, 1:3] = rng.uniform(lo, hi, (len(packed.knots), 2))  # every entity stands somewhere on the network's extent
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([a], np.zeros(R, np.int32))
    stream = torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    cap = 32
    count = torch.empty((R, E), dtype=torch.int32, device="cuda:0")
    geoms = torch.empty((R, E, cap), dtype=torch.int32, device="cuda:0")
    layers = torch.empty((R, E), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    q = lambda: eng.lib.sg_road_info(eng.h, cap, count.data_ptr(), geoms.data_ptr(), layers.data_ptr(), 1)  # noqa: E731
    ms = median_ms(q)
    c = count.cpu().numpy()
    lay = np.ascontiguousarray([1, 2, 4, 8, 16, 32, 64, 0], np.int32)
    import ctypes

    ptr = ctypes.c_void_p()
    m = lambda: eng.lib.sg_raster_map_device(eng.h, 20.0, 20.0, 20, 20, 8, lay.ctypes.data, ctypes.byref(ptr))  # noqa: E731
    ms_map = median_ms(m)
    print(f"{net}: sg_road_info {R} x {E} entities, device outputs, cap {cap}: median {ms[0]*1e3:.0f} us (min {ms[1]*1e3:.0f}, max {ms[2]*1e3:.0f}) "
          f"= {R*E/ms[0]/1e6:.2f} G queries/s; mean {c[c >= 0].mean():.2f} geometries per entity, max {c.max()}, {100*(c > 0).mean():.0f} % in some; "
          f"sg_raster_map_device 20 x 20 x 8 layers on the same batch ({R*400} point tests): median {ms_map[0]*1e3:.0f} us (min {ms_map[1]*1e3:.0f}, max {ms_map[2]*1e3:.0f})")
    eng.close()
