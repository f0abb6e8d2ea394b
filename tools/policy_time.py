"""Time of one tick with the built-in driver policy in the loop (sg_step_drivers_policy) beside one tick of sg_step_drivers on a
second handle with the same batch and the same driver list -- the path the library had before and the yardstick -- and the time
of the policy's launch alone (sg_driver_policy_actions with device outputs).
HIP events on the handle's stream around each call, warm, the calls interleaved in one process, median of 20 with min / max.
    python tools/policy_time.py [straight]
4096 x 64, device actions, every driver run by the policy along its own 16-point recording: 1. 8 drivers per scenario; 2. 63.
Writes profiles/driver_policy_time.json.  Then (not with `straight`, which is what an A/B run of two builds of the library asks for)
the same two cases with every driver in the corridor along its path (SG_DP_CORRIDOR == 1), and 2048 x 64 with 8 drivers per scenario
on paths of 1,024 points -- the recording, every segment cut into equal pieces -- in either mode, and along the path with REACH 80
and with REACH inf: the window of the corridor is its trip count.  Writes all of it to profiles/policy_corridor_time.json."""
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


def long_path(p, n):
    """The polyline p drawn with n points: its vertices kept, every segment cut into equal pieces."""
    u = np.linspace(0.0, len(p) - 1.0, n)
    return np.stack([np.interp(u, np.arange(len(p)), p[:, 0]), np.interp(u, np.arange(len(p)), p[:, 1])], 1)


def case(name, per_scenario, corridor="straight", path_points=16, reach=80.0, R=R):
    packed = synthetic.make_batch(R, E, n_steps=400, timestep=0.1, n_knots=16, ego_kind=L.KIND_AGENT_VEHICLE, seed=5)
    kinds = packed.kind.reshape(R, E).copy()
    kinds[:, E - per_scenario:] = L.KIND_AGENT_EXTERNAL  # (the ego, slot 0, stays what it is)
    packed.kind = kinds.ravel()
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(E - per_scenario, E), R)
    base, eng = sga.RolloutEngine(R, E, timestep=0.1), sga.RolloutEngine(R, E, timestep=0.1)
    for e_ in (base, eng):
        e_.upload(packed)
        e_.set_drivers(scen, slot)
    idx = scen.astype(np.int64) * E + slot
    # the batch of tools/drivers_time.py: a recording of fewer than 16 knots (static, vanishing) is padded with its last point
    recs = [packed.knots[packed.knot_off[i]:packed.knot_off[i + 1], 1:3] for i in idx]
    paths = [np.concatenate([p, np.repeat(p[-1:], 16 - len(p), axis=0)]) for p in recs]
    assert all(p.shape == (16, 2) for p in paths)
    if path_points != 16:
        paths = [long_path(p, path_points) for p in paths]
    eng.set_driver_policy(np.arange(len(scen)), np.tile(sga.idm_params(v0=10.0, reach=reach, corridor=corridor), (len(scen), 1)), paths)
    rng = np.random.default_rng(3)
    acts = torch.as_tensor(np.stack([rng.uniform(-2, 2, len(scen)), rng.uniform(-0.3, 0.3, len(scen))], -1), device="cuda:0").contiguous()
    out_act = torch.empty((len(scen), 2), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    s_base, s_eng = torch.cuda.ExternalStream(base.lib.sg_stream(base.h)), torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    f_base = lambda: base.lib.sg_step_drivers(base.h, 1, acts.data_ptr(), 1)  # noqa: E731
    f_pol = lambda: eng.lib.sg_step_drivers_policy(eng.h, 1, acts.data_ptr(), 1)  # noqa: E731
    f_act = lambda: eng.lib.sg_driver_policy_actions(eng.h, out_act.data_ptr(), None, None, 1)  # noqa: E731
    for _ in range(3):
        assert f_base() == 0 and f_pol() == 0 and f_act() == 0
    t_base, t_pol, t_act = [], [], []
    for _ in range(20):
        t_base.append(timed(s_base, f_base))
        t_pol.append(timed(s_eng, f_pol))
        t_act.append(timed(s_eng, f_act))
    out = dict(shape=[R, E], drivers=len(scen), policy_drivers_per_scenario=per_scenario, path_points=path_points, corridor=corridor, reach=reach,
               leads=int((eng.driver_policy_actions()[1][:, 0] >= 0).sum()), step_drivers_policy=summary(t_pol),
               step_drivers=summary(t_base), policy_launch=summary(t_act), difference_us=float(np.median(t_pol) - np.median(t_base)),
               policy_over_drivers=float(np.median(t_pol) / np.median(t_base)), kernel=eng.last_kernel())
    print(f"{name}: {R} x {E}, {len(scen)} policy drivers, {out['leads']} with a lead: sg_step_drivers_policy median {out['step_drivers_policy']['median_us']:.0f} us (min "
          f"{out['step_drivers_policy']['min_us']:.0f}, max {out['step_drivers_policy']['max_us']:.0f}); sg_step_drivers median "
          f"{out['step_drivers']['median_us']:.0f} us (min {out['step_drivers']['min_us']:.0f}, max {out['step_drivers']['max_us']:.0f}); the "
          f"policy's launch alone {out['policy_launch']['median_us']:.0f} us; difference {out['difference_us']:.0f} us")
    eng.close()
    base.close()
    return out


def write(name, res):
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    res = dict(tool="tools/policy_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0),
               eight_per_scenario=case("8 policy drivers per scenario", 8), sixty_three_per_scenario=case("63 policy drivers per scenario", 63))
    write("driver_policy_time.json", res)
    if sys.argv[1:] != ["straight"]:
        res["eight_per_scenario_path"] = case("8 per scenario, along the path", 8, "path")
        res["sixty_three_per_scenario_path"] = case("63 per scenario, along the path", 63, "path")
        for key, kw in (("long_straight", dict(corridor="straight")), ("long_path_reach_80", dict(corridor="path")),
                        ("long_path_reach_inf", dict(corridor="path", reach=float("inf")))):
            res[key] = case(key + ", 1,024 points per path", 8, path_points=1024, R=2048, **kw)
        write("policy_corridor_time.json", res)
