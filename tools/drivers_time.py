"""Time of one tick with per-entity actions (sg_step_drivers) beside one tick of sg_step with per-scenario actions on the twin
batch -- the same scenarios with the ego as SG_KIND_AGENT_VEHICLE, which is the path the library had before and the yardstick.
HIP events on the handle's stream around each call (both calls wait for their stream before they return), warm, the calls
interleaved in one process, median of 20 with min / max.
    python tools/drivers_time.py
4096 x 64, device actions: 1. the ego as the only driver; 2. 8 drivers per scenario; 3. every entity a driver.
Writes profiles/drivers_time.json."""
import json
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic

R, E = 4096, 64


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def summary(x):
    x = np.asarray(x)
    return dict(median_us=float(np.median(x)), min_us=float(x.min()), max_us=float(x.max()), repeats=len(x))


def case(name, per_scenario):
    packed = synthetic.make_batch(R, E, n_steps=400, timestep=0.1, n_knots=16, ego_kind=L.KIND_AGENT_VEHICLE, seed=5)
    twin = sga.RolloutEngine(R, E, timestep=0.1)
    twin.upload(packed)
    kinds = packed.kind.reshape(R, E).copy()
    kinds[:, :per_scenario] = L.KIND_AGENT_EXTERNAL
    packed.kind = kinds.ravel()
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(per_scenario), R)
    eng.set_drivers(scen, slot)
    rng = np.random.default_rng(3)
    a_twin = torch.as_tensor(np.stack([rng.uniform(-2, 2, R), rng.uniform(-0.3, 0.3, R)], -1), device="cuda:0").contiguous()
    a_drv = torch.as_tensor(np.stack([rng.uniform(-2, 2, len(scen)), rng.uniform(-0.3, 0.3, len(scen))], -1), device="cuda:0").contiguous()
    torch.cuda.synchronize()
    s_twin, s_drv = torch.cuda.ExternalStream(twin.lib.sg_stream(twin.h)), torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    f_twin = lambda: twin.lib.sg_step(twin.h, 1, a_twin.data_ptr(), 1)  # noqa: E731
    f_drv = lambda: eng.lib.sg_step_drivers(eng.h, 1, a_drv.data_ptr(), 1)  # noqa: E731
    for _ in range(3):
        assert f_twin() == 0 and f_drv() == 0
    t_twin, t_drv = [], []
    for _ in range(20):
        t_twin.append(timed(s_twin, f_twin))
        t_drv.append(timed(s_drv, f_drv))
    out = dict(shape=[R, E], drivers=len(scen), drivers_per_scenario=per_scenario, step_drivers=summary(t_drv), step_twin=summary(t_twin),
               drivers_over_twin=float(np.median(t_drv) / np.median(t_twin)), kernel_twin=twin.last_kernel(), kernel_drivers=eng.last_kernel())
    print(f"{name}: {R} x {E}, {len(scen)} drivers: sg_step_drivers median {out['step_drivers']['median_us']:.0f} us (min "
          f"{out['step_drivers']['min_us']:.0f}, max {out['step_drivers']['max_us']:.0f}); sg_step on the twin median "
          f"{out['step_twin']['median_us']:.0f} us (min {out['step_twin']['min_us']:.0f}, max {out['step_twin']['max_us']:.0f}); ratio "
          f"{out['drivers_over_twin']:.2f}")
    eng.close()
    twin.close()
    return out


if __name__ == "__main__":
    res = dict(tool="tools/drivers_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0),
               ego_only=case("the ego as the only driver", 1), eight_per_scenario=case("8 drivers per scenario", 8),
               every_entity=case("every entity a driver", E))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "drivers_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
