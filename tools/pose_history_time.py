"""Kernel time of the pose-history observation (sg_pose_history_observers, device outputs) beside the nearest-entity observation
(sg_nearest_entities_observers) on the same handle and state: the history call selects exactly as the nearest call does and then
gathers (1 + k) * n_samples record rows per observer where the nearest call gathers k state rows.  HIP events on the handle's
stream, both warm, interleaved call by call, median of 20.
    python tools/pose_history_time.py [out.json] [bench_pair.json]
The bench's 4096 x 64 shape, stepped 64 times with a record of 65 rows, one observer per scenario (its ego), n_samples 16, stride 1,
k 8, radius inf.  Writes profiles/pose_history_time.json (or out.json); bench_pair.json, if given, is a JSON object that is stored
as it is under "bench_pair" (the result lines of one alternating `python bench.py` pair, parent and tree)."""
import json
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic

R, E, STEPS = 4096, 64, 64
H, STRIDE, K, RADIUS = 16, 1, 8, float("inf")
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


def case():
    global stream
    packed = synthetic.make_batch(R, E, n_steps=10000, n_knots=128, seed=5)
    eng = sga.RolloutEngine(R, E, record_capacity=STEPS + 1)
    eng.upload(packed)
    eng.step(STEPS)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    eng.set_observers(np.arange(R), packed.ego)
    dev = "cuda:0"
    hist = torch.empty((R, 1 + K, H, L.HIST_NFEAT), dtype=torch.float64, device=dev)
    feat = torch.empty((R, K, 8), dtype=torch.float64, device=dev)
    slots, count = torch.empty((2, R, K), dtype=torch.int32, device=dev), torch.empty((2, R), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    history = lambda: lib.sg_pose_history_observers(h, H, STRIDE, K, RADIUS, hist.data_ptr(), slots[0].data_ptr(), count[0].data_ptr(), 1)  # noqa: E731
    nearest = lambda: lib.sg_nearest_entities_observers(h, K, RADIUS, feat.data_ptr(), slots[1].data_ptr(), count[1].data_ptr(), 1)  # noqa: E731
    assert history() == 0 and nearest() == 0, lib.sg_last_error(h)
    with torch.cuda.stream(stream):
        t_hist, t_near = series([history, nearest])
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    valid = hist[..., 5] == 1.0
    out = dict(shape=[R, E], steps=STEPS, record_rows=STEPS + 1, record_bytes=(STEPS + 1) * 6 * R * eng._view.entity_stride * 8, observers=R,
               n_samples=H, stride=STRIDE, k=K, radius="inf", pose_history=summary(t_hist), nearest_entities=summary(t_near),
               history_over_nearest=float(np.median(t_hist) / np.median(t_near)), row_gathers_ratio=(1 + K) * H / K,
               bytes_written=dict(pose_history=hist.numel() * 8, nearest_entities=feat.numel() * 8),
               agreement=dict(slots_equal=bool(torch.equal(slots[0], slots[1])), count_equal=bool(torch.equal(count[0], count[1])),
                              sample0_equal=bool(torch.equal(hist[:, 1:, 0, :4], feat[..., :4])), valid_fraction=float(valid.float().mean()),
                              stale=int((count[0] == -2).sum())))
    print(f"{R} x {E}, {STEPS} steps, {R} observers, n_samples {H}, stride {STRIDE}, k {K}: pose_history_kernel median "
          f"{out['pose_history']['median_us']:.0f} us (min {out['pose_history']['min_us']:.0f}, max {out['pose_history']['max_us']:.0f}); "
          f"nearest_kernel median {out['nearest_entities']['median_us']:.0f} us (min {out['nearest_entities']['min_us']:.0f}, max "
          f"{out['nearest_entities']['max_us']:.0f}); ratio {out['history_over_nearest']:.1f} for {out['row_gathers_ratio']:.0f} x the row gathers; "
          f"{out['agreement']}")
    eng.close()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "pose_history_time.json")
    res = dict(tool="tools/pose_history_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0), observers_4096x64=case())
    if len(sys.argv) > 2:
        res["bench_pair"] = json.load(open(sys.argv[2]))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
