"""Kernel time of the nearest-entity vector observation (sg_nearest_entities / sg_nearest_entities_observers, device outputs)
beside the only thing the library offered before it: a torch `topk` over the sg_state_view tensors that produces the same
three outputs.  HIP events on the handle's stream, both warm, interleaved call by call, median of 20.
    python tools/nearest_time.py [k]
1. 4096 x 64, the ego of every scenario (4096 observers).
2. 1024 x 256, every entity an observer (262144 observers).
Writes profiles/nearest_entities_time.json.  The baseline is plain torch: gathers of the state rows, one [n, E] distance matrix,
torch.topk(largest=False), torch.sin / torch.cos; it is not tuned, and where it orders ties otherwise or rounds sin / cos
otherwise than the library the agreement figures below say so."""
import json
import os
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

import scenario_gym_amd as sga
import scenario_gym_amd._lib as L
from scenario_gym_amd import synthetic

K = int(sys.argv[1]) if len(sys.argv) > 1 else 8
RADIUS = 30.0
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


def torch_baseline(eng, bbox, scen, slot, k, radius):
    """A closure that computes (feat, slots, count) of the observers (scen, slot) with torch ops over the state view."""
    view = eng.torch_state()  # [n_blocks, block_rows, 64] fp64, zero-copy
    R, E, EP = eng.R, eng.E, eng._view.entity_stride
    dev = view.device
    scen, slot = torch.as_tensor(scen, dtype=torch.int64, device=dev), torch.as_tensor(slot, dtype=torch.int64, device=dev)
    box_l = torch.as_tensor(bbox[:, :, 1], device=dev)
    box_w = torch.as_tensor(bbox[:, :, 0], device=dev)
    ar = torch.arange(E, device=dev)
    rows = torch.arange(len(scen), device=dev)
    r2 = radius * radius

    def field(f):
        return view[:, f, :].reshape(-1)[:R * EP].reshape(R, EP)[:, :E]

    def run():
        x, y, h = field(L.F_POSE), field(L.F_POSE + 1), field(L.F_POSE + 3)
        vx, vy = field(L.F_VEL), field(L.F_VEL + 1)
        present = field(L.F_PRESENT).contiguous().view(torch.int64) != 0
        xo, yo, ho, vxo, vyo = x[scen, slot], y[scen, slot], h[scen, slot], vx[scen, slot], vy[scen, slot]
        s, c = torch.sin(ho)[:, None], torch.cos(ho)[:, None]
        dx, dy = x[scen] - xo[:, None], y[scen] - yo[:, None]
        d2 = dx * dx + dy * dy
        cand = present[scen] & (ar[None, :] != slot[:, None]) & torch.isfinite(d2) & (d2 <= r2)
        key = torch.where(cand, d2, torch.full_like(d2, float("inf")))
        val, idx = torch.topk(key, min(k, E), dim=1, largest=False, sorted=True)
        if k > E:
            val = torch.nn.functional.pad(val, (0, k - E), value=float("inf"))
            idx = torch.nn.functional.pad(idx, (0, k - E))
        ok = torch.isfinite(val) & present[scen, slot][:, None]
        r = scen[:, None].expand(-1, k)
        gdx, gdy = dx[rows[:, None], idx], dy[rows[:, None], idx]
        he = h[r, idx]
        se, ce = torch.sin(he), torch.cos(he)
        dvx, dvy = vx[r, idx] - vxo[:, None], vy[r, idx] - vyo[:, None]
        feat = torch.stack([gdx * c + gdy * s, gdy * c - gdx * s, ce * c + se * s, se * c - ce * s, dvx * c + dvy * s, dvy * c - dvx * s,
                            box_l[r, idx], box_w[r, idx]], dim=2)
        feat = torch.where(ok[:, :, None], feat, torch.zeros_like(feat))
        slots = torch.where(ok, idx, torch.full_like(idx, -1)).to(torch.int32)
        count = torch.where(present[scen, slot], cand.sum(dim=1), torch.full_like(scen, -1)).to(torch.int32)
        return feat, slots, count

    return run


def case(name, R, E, every_entity):
    global stream
    packed = synthetic.make_batch(R, E, n_steps=100, timestep=0.1, n_knots=16, extent=40.0, vanish_frac=0.3, seed=5)
    eng = sga.RolloutEngine(R, E, timestep=0.1)
    eng.upload(packed)
    eng.step(5)
    lib, h = eng.lib, eng.h
    stream = torch.cuda.ExternalStream(lib.sg_stream(h))
    if every_entity:
        scen, slot = np.repeat(np.arange(R), E), np.tile(np.arange(E), R)
        eng.set_observers(scen, slot)
        call = lib.sg_nearest_entities_observers
    else:
        scen, slot = np.arange(R), packed.ego
        call = lib.sg_nearest_entities
    n = len(scen)
    feat = torch.empty((n, K, 8), dtype=torch.float64, device="cuda:0")
    slots = torch.empty((n, K), dtype=torch.int32, device="cuda:0")
    count = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    kernel = lambda: call(h, K, RADIUS, feat.data_ptr(), slots.data_ptr(), count.data_ptr(), 1)  # noqa: E731
    base = torch_baseline(eng, packed.bbox.reshape(R, E, 4), scen, slot, K, RADIUS)
    with torch.cuda.stream(stream):
        t_kernel, t_torch = series([kernel, base])
        b_feat, b_slots, b_count = base()
    lib.sg_synchronize(h)
    torch.cuda.synchronize()
    out = dict(shape=[R, E], observers=n, k=K, radius=RADIUS, kernel=summary(t_kernel), torch_topk=summary(t_torch),
               torch_over_kernel=float(np.median(t_torch) / np.median(t_kernel)),
               agreement=dict(count_equal=bool(torch.equal(count, b_count)), slots_equal_fraction=float((slots == b_slots).float().mean()),
                              feat_max_abs_diff_where_slots_equal=float(((feat - b_feat).abs() * (slots == b_slots)[:, :, None]).max()),
                              mean_count=float(count.float().mean())))
    print(f"{name}: {R} x {E}, {n} observers, k = {K}, radius {RADIUS}: nearest_kernel median {out['kernel']['median_us']:.0f} us "
          f"(min {out['kernel']['min_us']:.0f}, max {out['kernel']['max_us']:.0f}); torch topk median {out['torch_topk']['median_us']:.0f} us "
          f"(min {out['torch_topk']['min_us']:.0f}, max {out['torch_topk']['max_us']:.0f}); torch / kernel {out['torch_over_kernel']:.1f}; "
          f"{out['agreement']}")
    eng.close()
    return out


if __name__ == "__main__":
    res = dict(tool="tools/nearest_time.py", src_sha16=L.source_sha16(), device=torch.cuda.get_device_name(0),
               egos_4096x64=case("egos", 4096, 64, False), every_entity_1024x256=case("every entity", 1024, 256, True))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "nearest_entities_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
