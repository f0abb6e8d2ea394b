"""Kernel time of the time to collision (sg_time_to_collision_observers, device outputs) beside the entity status
(sg_entity_status_observers, device outputs) on the same handle, the same observers and the same state: per pair the one does four
slabs where the other does 32 point-to-segment distances, so the status is the yardstick.  HIP events on the handle's stream, all
warm, the two interleaved call by call, median / min / max of 20.
    python tools/ttc_time.py [output.json]
1. 4096 x 64 on the 6-lane intersection with the ego of every scenario as the observers, then 8 observers per scenario.
2. 256 x 600 (beyond the 512-slot tiles), the same two lists.
3. tools/status_time.py's own measurement of 4096 x 64 in the same session, unchanged.
Writes profiles/ttc_time.json."""
import json
import os
import sys

sys.path.insert(0, '.')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import scenario_gym_amd._lib as L
import status_time as ST

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "ttc_time.json")
HORIZON = 5.0


def observers(eng, R, per_scenario, name):
    """The time to collision of per_scenario observers per scenario (slots 0 .. per_scenario - 1) beside their status."""
    lib, h = eng.lib, eng.h
    scen, slot = np.repeat(np.arange(R), per_scenario), np.tile(np.arange(per_scenario), R)
    eng.set_observers(scen, slot)
    n, dev = len(scen), "cuda:0"
    feat, info = torch.empty((n, L.TTC_NFEAT), dtype=torch.float64, device=dev), torch.empty((n, L.TTC_NINFO), dtype=torch.int32, device=dev)
    s_flags, s_info = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, L.ST_NINFO), dtype=torch.int32, device=dev)
    s_feat = torch.empty((n, L.ST_NFEAT), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ttc = lambda: lib.sg_time_to_collision_observers(h, HORIZON, feat.data_ptr(), info.data_ptr(), 1)  # noqa: E731
    status = lambda: lib.sg_entity_status_observers(h, s_flags.data_ptr(), s_info.data_ptr(), s_feat.data_ptr(), 1)  # noqa: E731
    assert ttc() == 0 and status() == 0
    with torch.cuda.stream(ST.stream):
        t_ttc, t_status = ST.series([ttc, status])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    x, i = feat.cpu().numpy(), info.cpu().numpy()
    here, threat = i[:, 1] >= 0, i[:, 0] >= 0
    d = dict(observers=n, horizon=HORIZON, time_to_collision=ST.summary(t_ttc), entity_status=ST.summary(t_status),
             ratio_of_medians=float(np.median(t_ttc) / np.median(t_status)), present=float(here.mean()), with_a_threat=float(threat[here].mean()),
             overlapping_now=float((i[threat, 2] < 0).mean()) if threat.any() else 0.0,
             median_ttc=float(np.median(x[threat, 0])) if threat.any() else None, mean_contacts=float(i[here, 1].mean()))
    print(f"  {name} ({n} observers): sg_time_to_collision_observers median {d['time_to_collision']['median_us']:.0f} us (min "
          f"{d['time_to_collision']['min_us']:.0f}, max {d['time_to_collision']['max_us']:.0f}); sg_entity_status_observers "
          f"{d['entity_status']['median_us']:.0f} us; {d['with_a_threat']:.0%} of the present observers have a threat within {HORIZON} s, "
          f"{d['mean_contacts']:.2f} contacts each")
    return d


def batch(R, E, rn):
    eng, extent = ST.engine(R, E, rn)
    eng.step(5)
    ST.stream = torch.cuda.ExternalStream(eng.lib.sg_stream(eng.h))
    print(f"{R} x {E} on {ST.NETWORK} (extent {extent:.0f} m):")
    res = dict(shape=[R, E], network=ST.NETWORK, extent=extent, egos=observers(eng, R, 1, "the egos"),
               eight_per_scenario=observers(eng, R, 8, "8 observers per scenario"))
    eng.close()
    return res


if __name__ == "__main__":
    rn = ST.network()
    out = dict(tool="tools/ttc_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), batch_4096x64=batch(4096, 64, rn),
               batch_256x600=batch(256, 600, rn), status_time_batch_4096x64=ST.batch(4096, 64, rn))
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
