"""Kernel time of the surface scan (sg_surface_scan / sg_surface_scan_observers, device outputs) beside the yardstick the code
base already has for point tests against the road surfaces -- sg_raster_map_observers of one 64 x 64 surface layer, the same
4096 point tests per observer as 64 beams x (48 + 16) lookups -- and beside sg_range_scan at 64 beams, the other half of the
lidar.  HIP events on the handle's stream, all warm, interleaved call by call, median / min / max of 20.
    python tools/surface_scan_time.py [output.json]
4096 x 64 on the 6-lane intersection (tools/range_scan_time.py's batch), the ego of every scenario, then 8 observers per scenario:
  64 beams x 1 layer (driveable_surface), 48 steps of 0.5 m and 16 bisections;
  16 beams x 3 layers (driveable_surface, road, intersection), the same march;
  64 beams x 1 layer without bisections: the march alone.
Writes profiles/surface_scan_time.json."""
import json
import os
import sys

sys.path.insert(0, '.')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import range_scan_time as RS
import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic
from scenario_gym_amd.road_network import LAYER_DRIVEABLE, LAYER_INTERSECTION, LAYER_ROAD

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "surface_scan_time.json")
STEP, N_STEPS, N_REFINE, PX = 0.5, 48, 16, 64
SHAPES = (("64_beams_1_layer", 64, (LAYER_DRIVEABLE,), N_REFINE), ("16_beams_3_layers", 16, (LAYER_DRIVEABLE, LAYER_ROAD, LAYER_INTERSECTION), N_REFINE),
          ("64_beams_1_layer_march_only", 64, (LAYER_DRIVEABLE,), 0))  # (the last: what the bisections of the first cost)


def surface(lib, h, n, n_rays, bits, n_refine, observers):
    """(the call, its output tensors) of one scan configuration with device outputs."""
    lay = np.array(bits, np.int32)
    feat = torch.empty((n, len(lay), n_rays), dtype=torch.float64, device="cuda:0")
    flags = torch.empty((n, len(lay), n_rays), dtype=torch.uint8, device="cuda:0")
    hits = torch.empty((n, len(lay)), dtype=torch.int32, device="cuda:0")
    fn = lib.sg_surface_scan_observers if observers else lib.sg_surface_scan
    call = lambda: fn(h, len(lay), lay.ctypes.data, n_rays, -np.pi, 2.0 * np.pi / n_rays, STEP, N_STEPS, n_refine, feat.data_ptr(),  # noqa: E731
                      flags.data_ptr(), hits.data_ptr(), 1)
    return call, (feat, flags, hits, n_refine)


def told(name, t, outs, n_rays):
    feat, flags, hits, n_refine = outs
    here = hits[:, 0] >= 0
    d = dict(RS.summary(t), present=float(here.float().mean()), hit_fraction=float(hits[here].float().mean() / n_rays),
             on_the_layer=float(((flags[here][:, :, 0] & L.SURF_INSIDE) != 0).float().mean()),
             bisections_per_observer=float(hits[here].float().sum(1).mean()) * n_refine)
    print(f"  {name}: median {d['median_us']:.0f} us (min {d['min_us']:.0f}, max {d['max_us']:.0f}); {d['hit_fraction']:.0%} of the beams change side, "
          f"{d['on_the_layer']:.0%} of the observers stand on the layer")
    return d


def batch(eng, R, per_scenario, name):
    """The scans of per_scenario observers per scenario (slots 0 .. per_scenario - 1; slot 0 is the ego) beside the map raster of
    one 64 x 64 surface layer for the same observers and the range scan at 64 beams."""
    lib, h = eng.lib, eng.h
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(per_scenario), R)
    eng.set_observers(scen, slot)
    n, egos = len(scen), per_scenario == 1
    scans = [surface(lib, h, n, n_rays, bits, n_refine, observers=not egos) for _, n_rays, bits, n_refine in SHAPES]
    raster = torch.empty((n, 1, PX, PX), dtype=torch.uint8, device="cuda:0")
    layer = np.array([LAYER_DRIVEABLE], np.int32)
    side = 2.0 * STEP * N_STEPS  # the square the beams reach
    map_call = lambda: lib.sg_raster_map_observers(h, side, side, PX, PX, 1, layer.ctypes.data, raster.data_ptr(), 1)  # noqa: E731
    r_feat = torch.empty((n, 64, 2), dtype=torch.float64, device="cuda:0")
    r_slots = torch.empty((n, 64), dtype=torch.int32, device="cuda:0")
    r_hits = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    range_fn = lib.sg_range_scan if egos else lib.sg_range_scan_observers
    range_call = lambda: range_fn(h, 64, -np.pi, 2.0 * np.pi / 64, STEP * N_STEPS, r_feat.data_ptr(), r_slots.data_ptr(), r_hits.data_ptr(), 1)  # noqa: E731
    torch.cuda.synchronize()
    calls = [c for c, _ in scans] + [map_call, range_call]
    assert all(c() == 0 for c in calls)
    with torch.cuda.stream(RS.stream):
        *t_scans, t_map, t_range = RS.series(calls)
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    print(f" {name} ({n} observers):")
    res = dict(observers=n)
    for (key, n_rays, bits, _), t, (_, outs) in zip(SHAPES, t_scans, scans):
        res[key] = told(key.replace("_", " "), t, outs, n_rays)
    res["map_raster_1x64x64"], res["range_scan_64_beams"] = RS.summary(t_map), RS.summary(t_range)
    res["scan_64x1_over_map_raster"] = float(np.median(t_scans[0]) / np.median(t_map))
    print(f"  sg_raster_map_observers 1 x {PX} x {PX} over {side:.0f} m: median {res['map_raster_1x64x64']['median_us']:.0f} us (min "
          f"{res['map_raster_1x64x64']['min_us']:.0f}, max {res['map_raster_1x64x64']['max_us']:.0f}); sg_range_scan 64 beams to {STEP * N_STEPS:.0f} m: "
          f"median {res['range_scan_64_beams']['median_us']:.0f} us; 64 x 1 scan / map raster {res['scan_64x1_over_map_raster']:.2f}")
    return res


if __name__ == "__main__":
    R, E = 4096, 64
    rn = RS.network()
    v = rn.polygon_arrays()["verts"]
    extent = float((v.max(0) - v.min(0)).min()) / 2
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=extent, vanish_frac=0.3, seed=5)
    packed.knots[:, 1:3] += (v.max(0) + v.min(0)) / 2
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.set_road_networks([rn.polygon_arrays()], np.zeros(R, np.int32))
    eng.step(5)
    RS.stream = torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    print(f"{R} x {E} on {RS.NETWORK} (extent {extent:.0f} m), step {STEP} m x {N_STEPS}, {N_REFINE} bisections:")
    out = dict(tool="tools/surface_scan_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), shape=[R, E], network=RS.NETWORK,
               extent=extent, step=STEP, n_steps=N_STEPS, n_refine=N_REFINE, egos=batch(eng, R, 1, "the egos"),
               eight_per_scenario=batch(eng, R, 8, "8 observers per scenario"))
    eng.close()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
