"""Time of a device snapshot (sg_snapshot_save / sg_snapshot_restore: one launch of snapshot_copy_kernel) beside the runtime's own
device-to-device copies of the same arrays and beside one step of the same batch.  HIP events on the handles' streams, all warm, the
variants called in turn round by round, median / min / max of 20 and the spread (max - min over the median).
    python tools/snapshot_time.py [output.json]
Two handles hold the same batch: one copies a NULL-mask save / restore with the kernel, the other (created under SG_SNAP_D2D=1) with
one hipMemcpyAsync per state array on the same stream -- the baseline, the runtime's code and not ours.
1. 4096 x 64, the headline batch (a PID ego among replayed vehicles).
2. 1024 x 256, the crowd of config 5.
Per shape: bytes per snapshot; full save and full restore, kernel and copies; a restore of half the scenarios with the mask
alternating and with it contiguous (device masks); one sg_step.  Writes profiles/snapshot_time.json."""
import json
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "snapshot_time.json")
ROUNDS, WARM = 20, 3


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    assert fn() == 0
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def summary(x, moved):
    x = np.array(x)
    med = float(np.median(x))
    return dict(median_us=med, min_us=float(x.min()), max_us=float(x.max()), spread=float((x.max() - x.min()) / med), repeats=len(x),
                bytes_moved=int(moved), gb_per_s_read_plus_write=float(2 * moved / med / 1e3))


def engine(packed, d2d):
    os.environ["SG_SNAP_D2D"] = "1" if d2d else "0"
    eng = sga.RolloutEngine(packed.n_scenarios, packed.n_entities, timestep=1 / 30)
    eng.upload(packed)
    eng.step(5)
    return eng


def shape(name, packed):
    R = packed.n_scenarios
    ker, cpy = engine(packed, False), engine(packed, True)
    sk, sc = ker.snapshot(), cpy.snapshot()
    nbytes = sk.nbytes
    assert sc.nbytes == nbytes
    streams = {id(e): torch.cuda.ExternalStream(e.lib.sg_stream(e.h)) for e in (ker, cpy)}
    alt = torch.as_tensor((np.arange(R) % 2 == 0).astype(np.uint8), device="cuda:0")
    half = torch.as_tensor((np.arange(R) < R // 2).astype(np.uint8), device="cuda:0")
    torch.cuda.synchronize()
    lib = ker.lib
    variants = {  # name: (engine, call, share of the snapshot's bytes it moves)
        "save_kernel": (ker, lambda: lib.sg_snapshot_save(ker.h, sk._s, None, 0), 1.0),
        "save_copies": (cpy, lambda: lib.sg_snapshot_save(cpy.h, sc._s, None, 0), 1.0),
        "restore_kernel": (ker, lambda: lib.sg_snapshot_restore(ker.h, sk._s, None, 0), 1.0),
        "restore_copies": (cpy, lambda: lib.sg_snapshot_restore(cpy.h, sc._s, None, 0), 1.0),
        "restore_half_alternating": (ker, lambda: lib.sg_snapshot_restore(ker.h, sk._s, alt.data_ptr(), 1), 0.5),
        "restore_half_contiguous": (ker, lambda: lib.sg_snapshot_restore(ker.h, sk._s, half.data_ptr(), 1), 0.5),
        "one_sg_step": (ker, lambda: lib.sg_step(ker.h, 1, None, 0), 0.0),
    }
    times = {k: [] for k in variants}
    for rnd in range(WARM + ROUNDS):
        for k, (eng, fn, _) in variants.items():
            t = timed(streams[id(eng)], fn)
            if rnd >= WARM:
                times[k].append(t)
    res = dict(shape=[R, packed.n_entities], bytes_per_snapshot=nbytes)
    for k, (_, _, share) in variants.items():
        res[k] = summary(times[k], share * nbytes)
        print(f"  {name} {k:26s} median {res[k]['median_us']:8.1f} us (min {res[k]['min_us']:.1f}, max {res[k]['max_us']:.1f})"
              + (f"  {res[k]['gb_per_s_read_plus_write']:.0f} GB/s" if share else ""))
    for e in (ker, cpy):
        e.close()
    return res


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("snapshot_time.py: no GPU (nothing is measured without one)")
    out = dict(tool="tools/snapshot_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), rounds=ROUNDS)
    print("4096 x 64 (PID ego among replayed vehicles):")
    out["batch_4096x64"] = shape("4096x64", synthetic.make_batch(4096, 64, n_steps=400, n_knots=16, ego_kind=L.KIND_AGENT_PID, extent=60.0))
    print("1024 x 256 (the crowd of config 5):")
    out["batch_1024x256"] = shape("1024x256", synthetic.make_crowd(1024, 256, n_steps=400))
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
