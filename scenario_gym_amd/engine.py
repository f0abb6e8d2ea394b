"""RolloutEngine: thin object wrapper over one sg_handle (one GPU, R scenarios x E entity slots)."""
import ctypes as C
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib as L
from .obs_table import KINDS

TERMINAL_BITS = {"max_length": L.TERM_MAX_LENGTH, "collision": L.TERM_COLLISION,
                 "ego_collision": L.TERM_EGO_COLLISION, "ego_off_road": L.TERM_EGO_OFF_ROAD}

# VehicleController / PIDController constructor defaults (reference controller.py:64-70, 157-161)
SCEN_DTYPE = np.dtype([  # sg_scenario_state
    ("t", "f8"), ("prev_t", "f8"), ("ego_avg_speed", "f8"), ("ego_max_speed", "f8"), ("avg_t", "f8"),
    ("ego_distance_travelled", "f8"), ("last_row", "u8", (4,)), ("done", "i4"), ("n_steps", "i4"),
    ("n_events", "i4"), ("rec_rows", "i4"), ("noise_pos", "i8"), ("last_row_hi", "u8", (4,))])

# + PedestrianAgent / PedestrianController defaults (pedestrian/agent.py:18-27): speed_desired (set per agent),
# max_speed 5.0, head_rot_angle 0.0, distance_threshold 1.0
DEFAULT_CTRL = np.array([0.7, 5.0, np.nan, 0.0, 0.03054, 1.5709, 0.3753, 1.8970, 0.0204, 0.0, 5.0, 0.0, 1.0, 0, 0, 0])


@dataclass
class PackedScenarios:
    """Numeric content of R scenarios x E entity slots in the sg_scenarios layout."""

    n_scenarios: int
    n_entities: int
    kind: np.ndarray      # [R*E] int32
    etype: np.ndarray     # [R*E] int32
    bbox: np.ndarray      # [R*E, 4]
    knot_off: np.ndarray  # [R*E+1] int64
    knots: np.ndarray     # [rows, 7]
    ego: np.ndarray       # [R] int32
    t0: np.ndarray        # [R]
    length: np.ndarray    # [R]
    ctrl: Optional[np.ndarray] = None  # [R*E, 16]
    refs: list = field(default_factory=list)
    route_off: Optional[np.ndarray] = None  # [R*E+1] int64, pedestrian agents' waypoint rows
    routes: Optional[np.ndarray] = None     # [rows, 2]

    def validate(self):
        R, E = self.n_scenarios, self.n_entities
        assert self.kind.shape == (R * E,) and self.etype.shape == (R * E,)
        assert self.bbox.shape == (R * E, 4) and self.knot_off.shape == (R * E + 1,)
        assert self.knots.ndim == 2 and self.knots.shape[1] == 7
        assert self.ego.shape == (R,) and self.t0.shape == (R,) and self.length.shape == (R,)
        assert self.ctrl is None or self.ctrl.shape == (R * E, L.NCTRL)
        assert self.route_off is None or (self.route_off.shape == (R * E + 1,) and self.routes.shape[1] == 2)
        return self

    def pin(self, device=0):
        """Move the knots -- nearly all of the bytes of a batch -- into page-locked host memory (sg_host_alloc), in place:
        sg_upload then copies them at the PCIe rate without a staging copy on the host."""
        pinned = L.pinned_empty(self.knots.shape, np.float64, device)
        pinned[...] = self.knots
        self.knots = pinned
        return self

    def shard(self, lo, hi):
        """Scenarios [lo, hi) as an independent batch (replica sharding across GPUs)."""
        E = self.n_entities
        a, b = int(self.knot_off[lo * E]), int(self.knot_off[hi * E])
        ro = rt = None
        if self.route_off is not None:
            ra, rb = int(self.route_off[lo * E]), int(self.route_off[hi * E])
            ro, rt = self.route_off[lo * E:hi * E + 1] - ra, self.routes[ra:rb]
        return PackedScenarios(
            hi - lo, E, self.kind[lo * E:hi * E], self.etype[lo * E:hi * E], self.bbox[lo * E:hi * E],
            self.knot_off[lo * E:hi * E + 1] - a, self.knots[a:b], self.ego[lo:hi], self.t0[lo:hi],
            self.length[lo:hi], None if self.ctrl is None else self.ctrl[lo * E:hi * E],
            self.refs[lo:hi] if self.refs else [], ro, rt,
        )


def terminal_mask(conditions):
    if conditions is None:
        return L.TERM_MAX_LENGTH
    mask = 0
    for c in conditions:
        if c not in TERMINAL_BITS:
            raise ValueError(f"terminal condition {c!r} is not available on the device path "
                             f"(supported: {sorted(TERMINAL_BITS)})")
        mask |= TERMINAL_BITS[c]
    return mask


# SocialForceParameters (pedestrian/social_force.py:16-30): the model parameters of set_social_force / of a set_ped_models row
SOCIAL_FORCE_DEFAULTS = dict(relaxation_time=1.5, ped_repulse_V=1.0, ped_repulse_sigma=1.0, ped_attract_C=0.0, sight_weight=0.5,
                             sight_weight_use=True, sight_angle=200, max_speed_factor=1.3, bias_lon=0.0, bias_lat=0.0,
                             imp_boundary_repulse_U=2.0, imp_boundary_repulse_R=0.1)
_SF = SOCIAL_FORCE_DEFAULTS
PED_BEHAVIOURS = {"social_force": L.PED_SOCIAL_FORCE, "random_walk": L.PED_RANDOM_WALK}


def _social_force(who, params):
    """sg_social_force from set_social_force()'s parameter names; what `params` leaves out takes that method's default."""
    unknown = set(params) - set(SOCIAL_FORCE_DEFAULTS)
    if unknown:
        raise TypeError(f"{who}: unknown parameters {sorted(unknown)}")
    d = {**SOCIAL_FORCE_DEFAULTS, **params}
    d["sight_weight_use"] = float(bool(d["sight_weight_use"]))
    d["cos_sight"] = float(np.cos(d.pop("sight_angle") / 2 * np.pi / 180))
    return L.SgSocialForce(**d)


CORRIDORS = {"straight": 0.0, "path": 1.0}


def idm_params(v0, T=1.5, s0=2.0, a=1.5, b=2.0, half=0.2, reach=80.0, k_psi=1.0, k_e=0.5, k_soft=1.0, gap_min=0.1, corridor="straight"):
    """One parameter row of set_driver_policy ([DP_NPARAM] doubles): desired speed v0, time headway T, standstill gap s0, maximum
    acceleration a and comfortable deceleration b of the Intelligent Driver Model; the corridor's extra half width `half` and its
    length `reach` (inf: no limit); the steering gains on the heading error (k_psi) and on the lateral offset (k_e, softened by
    k_soft at low speed); the smallest gap the model divides by (gap_min); where the lead is looked for (corridor): "straight", a
    corridor in the driver's heading frame, or "path", a corridor bent along the driver's path (SG_DP_CORRIDOR of include/sgym.h)."""
    if corridor not in CORRIDORS:
        raise ValueError(f"idm_params: corridor={corridor!r} is none of {sorted(CORRIDORS)}")
    row = np.zeros(L.DP_NPARAM)
    row[[L.DP_V0, L.DP_T, L.DP_S0, L.DP_A, L.DP_B, L.DP_HALF, L.DP_REACH, L.DP_K_PSI, L.DP_K_E, L.DP_K_SOFT, L.DP_GAP_MIN, L.DP_CORRIDOR]] = (
        v0, T, s0, a, b, half, reach, k_psi, k_e, k_soft, gap_min, CORRIDORS[corridor])
    return row


class Snapshot:
    """One copy of an engine's state on the device (include/sgym.h, sg_snapshot_*): save() the rows of the masked scenarios into
    it, restore() them back; every later call then returns for those scenarios what it would have returned right after the save.
    mask: None (every scenario), a numpy bool / uint8 [R] array (copied before the call returns), or a torch uint8 / bool [R]
    tensor on the engine's GPU, read in stream order behind torch's current stream (ordered_with_torch) and to be left as it is
    until the copy has run.  Both calls are queued on the engine's stream and not waited for.  Settings (timestep, networks,
    observers, drivers, routes, policy) are not state.  After upload, set_drivers or a set_rss toggle a snapshot can only be
    closed."""

    def __init__(self, engine, handle):
        self.engine, self._s = engine, handle

    def _call(self, fn, mask):
        eng = self.engine
        if self._s is None:
            raise RuntimeError(f"{fn.__name__}: the snapshot is closed")
        if mask is None:
            eng._check(fn(eng.h, self._s, None, 0), fn.__name__)
        elif hasattr(mask, "data_ptr") and getattr(mask, "is_cuda", False):
            import torch

            assert mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and mask.numel() == eng.R
            with eng.ordered_with_torch():
                eng._check(fn(eng.h, self._s, mask.data_ptr(), 1), fn.__name__)
        else:
            m = np.ascontiguousarray(mask).astype(np.uint8, copy=False)
            assert m.shape == (eng.R,)
            eng._check(fn(eng.h, self._s, m.ctypes.data, 0), fn.__name__)

    def save(self, mask=None):
        self._call(self.engine.lib.sg_snapshot_save, mask)

    def restore(self, mask=None):
        self._call(self.engine.lib.sg_snapshot_restore, mask)

    @property
    def nbytes(self):
        n = C.c_uint64()
        self.engine._check(self.engine.lib.sg_snapshot_bytes(self.engine.h, self._s, C.byref(n)), "sg_snapshot_bytes")
        return int(n.value)

    def close(self):
        """Frees the snapshot (waits for the engine's stream); a second call does nothing."""
        s, self._s = self._s, None
        eng = self.engine
        if s is not None and getattr(eng, "h", None):
            snaps = eng.__dict__.get("_snapshots", [])
            if self in snaps:
                snaps.remove(self)
            eng._check(eng.lib.sg_snapshot_destroy(eng.h, s), "sg_snapshot_destroy")


class RolloutEngine:
    """ScenarioGym's step loop for a whole batch, resident on one MI355X."""

    idm_params = staticmethod(idm_params)

    def __init__(self, n_scenarios, n_entities, timestep=1.0 / 30.0, persist=False,
                 terminal_conditions=None, record_capacity=0, event_capacity=16, device=0, social_force=None):
        self.lib = L.load()
        self.R, self.E = int(n_scenarios), int(n_entities)
        self.cfg = L.SgConfig(int(device), self.R, self.E, int(bool(persist)),
                              terminal_mask(terminal_conditions), int(record_capacity),
                              int(event_capacity), 0, float(timestep))
        self.h = C.c_void_p()
        rc = self.lib.sg_create(C.byref(self.cfg), C.byref(self.h))
        if rc != L.SG_OK:
            msg = self.lib.sg_last_error(None).decode()
            self.h = None
            raise RuntimeError(f"sg_create failed ({rc}): {msg}")
        self._view = None
        self._keep = None
        self._n_obs = 0  # observers set (set_observers)
        self._n_drv = 0  # drivers set (set_drivers)
        if social_force is not None and "models" in social_force:  # per-agent models (BatchedScenarioGym)
            self.set_ped_models(social_force["models"], social_force.get("model_of"), noise=social_force.get("noise"),
                                noise_seed=social_force.get("noise_seed", 0), normals=social_force.get("normals"))
        elif social_force is not None:
            self.set_social_force(**social_force)

    def set_social_force(self, relaxation_time=_SF["relaxation_time"], ped_repulse_V=_SF["ped_repulse_V"],
                         ped_repulse_sigma=_SF["ped_repulse_sigma"], ped_attract_C=_SF["ped_attract_C"], sight_weight=_SF["sight_weight"],
                         sight_weight_use=_SF["sight_weight_use"], sight_angle=_SF["sight_angle"], max_speed_factor=_SF["max_speed_factor"],
                         bias_lon=_SF["bias_lon"], bias_lat=_SF["bias_lat"], imp_boundary_repulse_U=_SF["imp_boundary_repulse_U"],
                         imp_boundary_repulse_R=_SF["imp_boundary_repulse_R"],
                         std_lon=0.0, std_lat=0.0, noise=None, noise_seed=0, normals=None, behaviour="social_force"):
        """SocialForceParameters of every pedestrian agent on this handle (pedestrian/social_force.py:16-30);
        call before upload().  behaviour="random_walk": the pedestrians follow RandomWalk (pedestrian/random_walk.py:22-44)
        instead, which reads bias_lon / bias_lat / std_lon / std_lat only.  std_lon / std_lat with noise="device" (counter-based generator on the GPU, the default when
        a std is non-zero) or noise="stream" + normals[R, n] (the variates numpy's legacy generator would hand out:
        np.random.RandomState(k).standard_normal(n) per scenario) are the random fluctuations of :106-108."""
        sf = _social_force("set_social_force", dict(
            relaxation_time=relaxation_time, ped_repulse_V=ped_repulse_V, ped_repulse_sigma=ped_repulse_sigma, ped_attract_C=ped_attract_C,
            sight_weight=sight_weight, sight_weight_use=sight_weight_use, sight_angle=sight_angle, max_speed_factor=max_speed_factor,
            bias_lon=bias_lon, bias_lat=bias_lat, imp_boundary_repulse_U=imp_boundary_repulse_U, imp_boundary_repulse_R=imp_boundary_repulse_R))
        self._check(self.lib.sg_set_social_force(self.h, C.byref(sf)), "sg_set_social_force")
        self.set_ped_behaviour(behaviour)
        if noise is None:
            noise = "device" if (std_lon != 0 or std_lat != 0) else "off"
        self.set_ped_noise(noise, std_lon, std_lat, normals=normals, seed=noise_seed)

    def set_ped_models(self, models, model_of=None, noise=None, noise_seed=0, normals=None):
        """sg_set_ped_models: per-agent behaviour models (pedestrian/agent.py:18-41: every PedestrianAgent holds its own
        behaviour object).  models: dicts of set_social_force()'s parameter names (+ behaviour, std_lon, std_lat);
        model_of[R * E]: the model of every entity slot (ignored where there is no pedestrian agent).  The noise MODE is one
        per handle (noise = "off" / "device" / "stream" + normals; default: "device" when any std is non-zero); before upload()."""
        rows = (L.SgPedModel * len(models))()
        any_std = False
        for i, m in enumerate(models):
            m = dict(m)
            beh = m.pop("behaviour", "social_force")
            std_lon, std_lat = float(m.pop("std_lon", 0.0)), float(m.pop("std_lat", 0.0))
            for k in ("noise", "noise_seed", "normals"):
                m.pop(k, None)
            rows[i].params = _social_force("set_ped_models", m)
            rows[i].behaviour = PED_BEHAVIOURS[beh]
            rows[i].std_lon, rows[i].std_lat = std_lon, std_lat
            any_std = any_std or std_lon != 0 or std_lat != 0
        if noise is None:
            noise = "device" if any_std else "off"
        # the mode first (its std arguments are those of a one-model handle; the models carry their own)
        self.set_ped_noise(noise, rows[0].std_lon, rows[0].std_lat, normals=normals, seed=noise_seed)
        mo = None
        if model_of is not None:
            mo = np.ascontiguousarray(model_of, np.int32).ravel()
            if mo.size != self.R * self.E:
                raise ValueError(f"model_of must have n_scenarios * n_entities = {self.R * self.E} entries")
        self._check(self.lib.sg_set_ped_models(self.h, len(models), rows, None if mo is None else mo.ctypes.data), "sg_set_ped_models")

    def set_ped_behaviour(self, behaviour="social_force"):
        """sg_set_ped_behaviour: "social_force" or "random_walk" for every pedestrian agent of the handle; before upload()."""
        self._check(self.lib.sg_set_ped_behaviour(self.h, PED_BEHAVIOURS[behaviour]), "sg_set_ped_behaviour")

    def set_ped_noise(self, mode="off", std_lon=0.0, std_lat=0.0, normals=None, seed=0):
        """sg_set_ped_noise: "off", "stream" (normals[R, n] standard normal variates per scenario) or "device"."""
        code = {"off": L.NOISE_OFF, "stream": L.NOISE_STREAM, "device": L.NOISE_DEVICE}[mode]
        ptr, n = None, 0
        if code == L.NOISE_STREAM:
            normals = np.ascontiguousarray(normals, np.float64)
            if normals.ndim != 2 or normals.shape[0] != self.R:
                raise ValueError(f"normals must be [n_scenarios = {self.R}, n]")
            ptr, n = normals.ctypes.data_as(C.c_void_p), normals.shape[1]
        self._check(self.lib.sg_set_ped_noise(self.h, code, float(std_lon), float(std_lat), ptr, int(n), int(seed) & (2 ** 64 - 1)),
                    "sg_set_ped_noise")

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc, what):
        if rc != L.SG_OK:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.sg_last_error(self.h).decode()}")

    def _outputs(self, torch_out, *specs):
        """One uninitialised output array per (shape, numpy dtype name, torch dtype name): numpy arrays, or with torch_out torch
        tensors in HBM that the handle's stream may write at once.  Returns (arrays, their addresses for the C side -- None for an
        empty array)."""
        if torch_out:
            import torch

            dev = f"cuda:{self.cfg.device}"
            arrs = tuple(torch.empty(shape, dtype=getattr(torch, dt), device=dev) for shape, _, dt in specs)
            torch.cuda.current_stream(arrs[0].device).synchronize()  # (the allocator's work before the handle's stream writes)
            return arrs, tuple(a.data_ptr() if a.numel() else None for a in arrs)
        arrs = tuple(np.empty(shape, dt) for shape, dt, _ in specs)
        return arrs, tuple(a.ctypes.data if a.size else None for a in arrs)

    def _actions(self, actions, n, rows=None, wait=True):
        """The actions of n ticks ([n, rows, 2], rows = R unless given: numpy, a float64 torch tensor on the device, or None) for
        the stepping calls: (the array the pointer points into, pointer, on_device).  wait=False: a tensor's writes are not waited
        for (the caller orders the streams)."""
        rows = self.R if rows is None else rows
        if actions is None:
            return None, None, 0
        if hasattr(actions, "data_ptr") and getattr(actions, "is_cuda", False):
            # a torch tensor on this GPU (fp64, contiguous): its device pointer goes down as it is
            import torch

            assert actions.dtype == torch.float64 and actions.is_contiguous() and actions.numel() == n * rows * 2
            if wait:
                torch.cuda.current_stream(actions.device).synchronize()  # the policy's writes before the handle's stream reads
            return actions, actions.data_ptr(), 1
        actions = np.ascontiguousarray(actions, np.float64).reshape(n, rows, 2)
        return actions, actions.ctypes.data, 0

    def _observe(self, call, args, torch_out, *specs):
        """The shared tail of the observation wrappers: the outputs of _outputs(torch_out, *specs), call(h, *args, their
        addresses, torch_out), and with torch_out the wait for the kernel (sg_synchronize: the C call itself does not wait)."""
        outs, ptrs = self._outputs(torch_out, *specs)
        self._check(call(self.h, *args, *ptrs, int(bool(torch_out))), call.__name__)
        if torch_out:
            self._check(self.lib.sg_synchronize(self.h), "sg_synchronize")
        return outs

    def _observation(self, kind, observers, user_args, torch_out=False, into=None, ordered=True):
        """Every observation of obs_table.KINDS, for the egos or the observers of set_observers, from its row: the C call of the
        pair, the arguments as the row casts them, the outputs the row describes.  Delivered as numpy arrays, with torch_out as
        torch tensors in HBM (waited for: _observe), or into the caller's tensors `into` -- checked against the row: on this
        GPU, dtype, contiguous, shape -- queued under ordered_with_torch(ordered) with no host wait."""
        row = KINDS[kind]
        call = getattr(self.lib, f"sg_{row.stem}_observers" if observers else f"sg_{row.stem}")
        args, _keep = row.args(*user_args)
        specs = row.outs(self._n_obs if observers else self.R, *args)
        if into is None:
            return self._observe(call, args, torch_out, *specs)
        import torch

        assert len(into) == len(specs)
        for t, (shape, _, dt) in zip(into, specs):
            assert t.is_cuda and t.device.index == self.cfg.device and t.dtype == getattr(torch, dt) and t.is_contiguous() and tuple(t.shape) == shape
        with self.ordered_with_torch(ordered):
            self._check(call(self.h, *args, *(t.data_ptr() if t.numel() else None for t in into), 1), call.__name__)
        return tuple(into)

    def _entity_list(self, scenario, slot, who):
        """The (scenario, slot) pairs of a list call: ((the int32 arrays), n, their addresses -- None for an empty list)."""
        scen = np.ascontiguousarray(scenario, np.int32).ravel()
        slot = np.ascontiguousarray(slot, np.int32).ravel()
        if scen.shape != slot.shape:
            raise ValueError(f"{who}: scenario and slot must have the same length")
        n = len(scen)
        return (scen, slot), n, scen.ctypes.data if n else None, slot.ctypes.data if n else None

    def _path_table(self, paths):
        """The polylines of a path call: ((the arrays), the address of pt_off [len(paths) + 1] int64, of pts [pt_off[-1], 2] or None)."""
        paths = [np.ascontiguousarray(q, np.float64).reshape(-1, 2) for q in paths]
        pt_off = np.concatenate([[0], np.cumsum([len(q) for q in paths])]).astype(np.int64)
        pts = np.ascontiguousarray(np.concatenate(paths, axis=0)) if pt_off[-1] else np.zeros((0, 2))
        return (pt_off, pts), pt_off.ctypes.data, pts.ctypes.data if len(pts) else None

    def _device_view(self, ptr, shape, typestr):
        """Zero-copy torch tensor over device memory of the handle."""
        import torch

        class _Arr:
            __cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)

        return torch.as_tensor(_Arr(), device=f"cuda:{self.cfg.device}")

    def close(self):
        if getattr(self, "h", None):
            for snap in list(self.__dict__.get("_snapshots", ())):
                snap.close()
            self.lib.sg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ ABI calls
    def upload(self, packed: PackedScenarios):
        packed.validate()
        if (packed.n_scenarios, packed.n_entities) != (self.R, self.E):
            raise ValueError("packed batch does not match the engine's (n_scenarios, n_entities)")
        arrs = dict(
            kind=np.ascontiguousarray(packed.kind, np.int32), etype=np.ascontiguousarray(packed.etype, np.int32),
            bbox=np.ascontiguousarray(packed.bbox, np.float64), knot_off=np.ascontiguousarray(packed.knot_off, np.int64),
            knots=np.ascontiguousarray(packed.knots, np.float64),
            ctrl=None if packed.ctrl is None else np.ascontiguousarray(packed.ctrl, np.float64),
            ego=np.ascontiguousarray(packed.ego, np.int32), t0=np.ascontiguousarray(packed.t0, np.float64),
            length=np.ascontiguousarray(packed.length, np.float64),
            route_off=None if packed.route_off is None else np.ascontiguousarray(packed.route_off, np.int64),
            routes=None if packed.routes is None else np.ascontiguousarray(packed.routes, np.float64),
        )
        sc = L.SgScenarios(*[None if arrs[n] is None else arrs[n].ctypes.data for n, _ in L.SgScenarios._fields_])
        self._n_obs = 0  # (sg_upload forgets the observers)
        self._n_drv = 0  # (... and the drivers)
        self._n_pol = 0  # (... and their policy)
        self._check(self.lib.sg_upload(self.h, C.byref(sc)), "sg_upload")
        self._view = L.SgStateView()
        self._check(self.lib.sg_state_view_get(self.h, C.byref(self._view)), "sg_state_view_get")
        return self

    def reset(self):
        self._check(self.lib.sg_reset(self.h), "sg_reset")

    def set_timestep(self, dt):
        self._check(self.lib.sg_set_timestep(self.h, float(dt)), "sg_set_timestep")

    def step(self, n_steps=1, actions=None):
        """n x ScenarioGym.step(); actions [n, R, 2] (accel, steer) for external-action slots."""
        _keep, ptr, on_device = self._actions(actions, n_steps)
        self._check(self.lib.sg_step(self.h, int(n_steps), ptr, on_device), "sg_step")

    def set_external_poses(self, poses):
        """Poses [R, E, 6] of the caller-run agents (KIND_AGENT_EXTERNAL slots; NaN x = the agent returned None)."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(self.R, self.E, 6)
        self._check(self.lib.sg_set_external_poses(self.h, poses.ctypes.data), "sg_set_external_poses")

    def set_drivers(self, scenario, slot):
        """sg_set_drivers: the policy-driven vehicles of step_drivers -- driver k is entity slot slot[k] of scenario
        scenario[k], a KIND_AGENT_EXTERNAL slot whose VehicleController (its ctrl row) the device runs itself.  Any number per
        scenario, no pair twice; the order is the order of the actions.  An empty list clears it; upload() forgets it; a
        refused list leaves the previous one in place."""
        _keep, n, p_scen, p_slot = self._entity_list(scenario, slot, "set_drivers")
        self._check(self.lib.sg_set_drivers(self.h, n, p_scen, p_slot), "sg_set_drivers")
        self._n_drv = n
        self._n_pol = 0  # (sg_set_drivers forgets the policy)

    def step_drivers(self, actions=None, n=1):
        """n x ScenarioGym.step() with the drivers' controllers run on the device (sg_step_drivers): actions [n, n_drivers, 2]
        (accel, steer) in the order of set_drivers -- numpy, a float64 torch tensor on the device, or None for (0, 0)."""
        _keep, ptr, on_device = self._actions(actions, int(n), getattr(self, "_n_drv", 0))
        self._check(self.lib.sg_step_drivers(self.h, int(n), ptr, on_device), "sg_step_drivers")

    def set_driver_policy(self, driver, params, paths):
        """sg_set_driver_policy: the built-in policy (IDM car-following along a path) runs driver[j] of the set_drivers list with
        the parameter row params[j] (idm_params) along paths[j], a [k, 2] array of x, y in driving order.  driver: positions in
        the driver list, strictly ascending.  An empty list clears the policy; set_drivers and upload() forget it; a refused
        call leaves the previous one in place."""
        driver = np.ascontiguousarray(driver, np.int64).ravel()
        m = len(driver)
        if m == 0:
            self._check(self.lib.sg_set_driver_policy(self.h, None), "sg_set_driver_policy")
            self._n_pol = 0
            return
        params = np.ascontiguousarray(params, np.float64).reshape(m, L.DP_NPARAM)
        if len(paths) != m:
            raise ValueError("set_driver_policy: one path per policy driver")
        _keep, p_off, p_pts = self._path_table(paths)
        pol = L.SgDriverPolicy(m, driver.ctypes.data, params.ctypes.data, p_off, p_pts)
        self._check(self.lib.sg_set_driver_policy(self.h, C.byref(pol)), "sg_set_driver_policy")
        self._n_pol = m

    def driver_policy_actions(self, torch_out=False):
        """The policy of set_driver_policy evaluated on the current state (sg_driver_policy_actions): (actions [m, 2] (accel,
        steer), info [m, 2] the lead's slot and the best path segment (-1: none), feat [m, 6] gap, closing speed, lateral offset,
        sine of the heading error, arclength along the path, remaining path).  Empty arrays when no policy is set.  torch_out:
        torch tensors in HBM the kernel writes directly (waited for, as in entity_status)."""
        m = getattr(self, "_n_pol", 0)
        return self._observe(self.lib.sg_driver_policy_actions, (), torch_out, ((m, 2), "float64", "float64"), ((m, L.DP_NINFO), "int32", "int32"),
                             ((m, L.DP_NFEAT), "float64", "float64"))

    def step_drivers_policy(self, actions=None, n=1):
        """step_drivers with the built-in policy in the loop (sg_step_drivers_policy): actions [n, n_drivers, 2] as for
        step_drivers; ahead of every step the rows of the policy drivers are replaced, in a buffer of the handle, by the policy
        evaluated on the state before that step.  The caller's array is never written."""
        _keep, ptr, on_device = self._actions(actions, int(n), getattr(self, "_n_drv", 0))
        self._check(self.lib.sg_step_drivers_policy(self.h, int(n), ptr, on_device), "sg_step_drivers_policy")

    def future_collision(self, horizon=5.0, n_samples=10):
        """FutureCollisionDetector (sensor/common.py:59-106) for the ego of every scenario at the current time: bool [R]."""
        out = np.zeros(self.R, np.uint8)
        self._check(self.lib.sg_future_collision(self.h, float(horizon), int(n_samples), out.ctypes.data), "sg_future_collision")
        return out.astype(bool)

    def raster_entities(self, width=20.0, height=20.0, nw=20, nh=20):
        """RasterizedMapSensor "entity" layer (sensor/map.py:120-192) around the ego of every scenario: bool [R, nh, nw]."""
        out = np.zeros((self.R, int(nh), int(nw)), np.uint8)
        self._check(self.lib.sg_raster_entities(self.h, float(width), float(height), int(nw), int(nh), out.ctypes.data),
                    "sg_raster_entities")
        return out.astype(bool)

    def reset_scenarios(self, mask):
        """State.reset for the scenarios with mask[r] != 0; the others keep their state."""
        m = np.ascontiguousarray(mask, np.uint8)
        assert m.shape == (self.R,)
        self._check(self.lib.sg_reset_scenarios(self.h, m.ctypes.data), "sg_reset_scenarios")

    def reset_scenarios_device(self, mask):
        """reset_scenarios with the mask on the device (sg_reset_scenarios_device): a torch uint8 (or bool) tensor [R] on this
        GPU.  Queued on the engine's stream behind the work of torch's current stream, not waited for; the tensor must stay as
        it is until the reset has run (work queued on torch's current stream after this call is ordered behind it)."""
        import torch

        assert mask.is_cuda and mask.dtype in (torch.uint8, torch.bool) and mask.is_contiguous() and mask.numel() == self.R
        with self.ordered_with_torch():
            self._check(self.lib.sg_reset_scenarios_device(self.h, mask.data_ptr()), "sg_reset_scenarios_device")

    def snapshot(self):
        """A Snapshot of the engine's state as it is now (sg_snapshot_create): every scenario saved.  Allocates, so it may wait
        for the device; save / restore never do."""
        s = C.c_void_p()
        self._check(self.lib.sg_snapshot_create(self.h, C.byref(s)), "sg_snapshot_create")
        snap = Snapshot(self, s)
        self.__dict__.setdefault("_snapshots", []).append(snap)
        return snap

    def _stream(self):
        """The engine's stream (sg_stream) as a torch stream: what orders it against torch's streams without a host wait."""
        import torch

        if self.__dict__.get("_ext_stream") is None:
            self._ext_stream = torch.cuda.ExternalStream(self.lib.sg_stream(self.h), device=f"cuda:{self.cfg.device}")
        return self._ext_stream

    @contextmanager
    def ordered_with_torch(self, enabled=True):
        """What is queued on the engine's stream inside the block runs behind the work torch's current stream holds at its start,
        and what torch's current stream gets after the block runs behind that: two events, no host wait.  Around several queued
        calls (tick_drivers, raster_map_observers_queued with ordered=False) it orders them as one."""
        if not enabled:
            yield
            return
        import torch

        ext, cur = self._stream(), torch.cuda.current_stream(torch.device(f"cuda:{self.cfg.device}"))
        ext.wait_stream(cur)
        try:
            yield
        finally:
            cur.wait_stream(ext)

    def tick_drivers(self, actions=None, terminal_mask=None, bad_env_flags=L.TERM_EGO_OFF_ROAD | L.TERM_EGO_COLLISION,
                     bad_driver_flags=L.ST_OFF_ROAD | L.ST_COLLISION, auto_reset=True, r_step=0.01, r_bad=-1.0, w_progress=0.0, ordered=True):
        """One tick of a multi-agent environment entirely on the device (sg_tick_drivers): the step of the drivers (the policy of
        set_driver_policy ahead of it), the terminal conditions, the drivers' status and -- with w_progress != 0 -- route rows,
        reward, done, progress and episode statistics per scenario and per driver, and with auto_reset the reset of the scenarios
        that finished.  actions [n_drivers, 2]: a float64 torch tensor on this GPU (read in stream order behind torch's current
        stream, no host wait), numpy (copied before the call returns), or None for (0, 0).  terminal_mask: the TERM_* bits that
        end an episode (None: the engine's terminal conditions).  Returns a dict of zero-copy torch views of the arrays of
        sg_episode_view -- term_flags, env_done, env_reward, reset_mask, ep_length [R]; drv_flags, drv_info, drv_feat, drv_progress,
        drv_reward, ep_return, drv_done [n_drivers, ...], and with w_progress != 0 drv_route, drv_route_info (else None) -- written
        in stream order: torch's current stream is ordered behind the tick, nothing waits on the host (ordered=False: the caller
        orders the two streams itself, ordered_with_torch).  The views are valid until the next tick_drivers, set_drivers or
        upload, and the same tensors come back while the addresses stay."""
        nd = getattr(self, "_n_drv", 0)
        _keep, ptr, on_device = self._actions(actions, 1, nd, wait=False)  # (a tensor is read in stream order: ordered_with_torch)
        rules = L.SgEpisodeRules(self.cfg.terminal_mask if terminal_mask is None else int(terminal_mask), int(bad_env_flags), int(bad_driver_flags),
                                 int(bool(auto_reset)), float(r_step), float(r_bad), float(w_progress))
        view = self.__dict__.setdefault("_ep_view", L.SgEpisodeView())
        with self.ordered_with_torch(ordered):  # the policy's writes before the tick, what the caller queues next behind it
            self._check(self.lib.sg_tick_drivers(self.h, ptr, on_device, C.byref(rules), C.byref(view)), "sg_tick_drivers")
        cache = self.__dict__.setdefault("_ep_views", {})
        out = {}
        for k, (name, typestr, cols) in enumerate(L.EPISODE_VIEW):
            p = getattr(view, name)
            if not p:
                out[name] = None
                continue
            rows = self.R if k < L.EPISODE_VIEW_PER_SCENARIO else nd
            key = (name, p, rows)
            if key not in cache:  # the buffer moved (first call, another driver list): wrap the new address once
                for old in [q for q in cache if q[0] == name]:
                    del cache[old]
                cache[key] = self._device_view(p, (rows, cols) if cols else (rows,), typestr)
            out[name] = cache[key]
        return out

    def terminal_flags(self):
        """TERM_* bits of every scenario's current state, all four conditions evaluated: uint32 [R]."""
        out = np.zeros(self.R, np.uint32)
        self._check(self.lib.sg_terminal_flags(self.h, out.ctypes.data, None), "sg_terminal_flags")
        return out

    def set_road_networks(self, networks, net_of_scenario):
        """Scenario.road_network of the uploaded batch.  networks: list of polygon_arrays() dicts (ring_off, vert_off, verts,
        layers; scenario_gym_amd.road_network.RoadNetwork), net_of_scenario: [R] index into it, -1 = no road network.
        Needed by the ego_off_road terminal condition and the surface layers of raster_map; call after upload()."""
        nos = np.ascontiguousarray(net_of_scenario, np.int32)
        assert nos.shape == (self.R,)
        poly_off, ring_off, vert_off, verts, layers = [0], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [], []
        n_ring = n_vert = 0
        for a in networks:
            ro, vo = np.asarray(a["ring_off"], np.int64), np.asarray(a["vert_off"], np.int64)
            ring_off.append(ro[1:] + n_ring)  # (running totals: a network without polygons or rings adds nothing)
            vert_off.append(vo[1:] + n_vert)
            n_ring, n_vert = n_ring + int(ro[-1]), n_vert + int(vo[-1])
            verts.append(np.asarray(a["verts"], np.float64).reshape(-1, 2))
            layers.append(np.asarray(a["layers"], np.uint32))
            poly_off.append(poly_off[-1] + len(a["layers"]))
        poly_off = np.array(poly_off, np.int64)
        ring_off, vert_off = np.concatenate(ring_off), np.concatenate(vert_off)
        verts = np.ascontiguousarray(np.concatenate(verts) if verts else np.zeros((0, 2)))
        layers = np.ascontiguousarray(np.concatenate(layers) if layers else np.zeros(0, np.uint32))
        p = lambda a: a.ctypes.data  # noqa: E731
        st = L.SgRoadNetworks(len(networks), p(nos), p(poly_off), p(ring_off), p(vert_off), p(verts), p(layers))
        self._check(self.lib.sg_set_road_networks(self.h, C.byref(st)), "sg_set_road_networks")

    def road_info(self, cap=32, torch_out=False):
        """State.get_road_info_at_entity (state/state.py:330-338) for every entity slot at its current pose (sg_road_info):
        (count [R, E] int32, geoms [R, E, cap] int32, layers [R, E]).  count = how many geometries of the scenario's network
        contain the entity (-1: the slot is not in State.poses; 0 without a network); geoms = their indices within the network
        as set_road_networks got it (`RoadNetwork.geometry_index` order), ascending, -1 behind the last; layers = the OR of
        their LAYER_* bits.  Host form: numpy arrays; when some entity lies in more than `cap` geometries the query is
        repeated once with cap = count.max(), so no list comes back truncated.  torch_out: torch tensors in HBM (int32;
        layers as int32 bit patterns) the kernel writes directly, ordered after it; lists stop at `cap` there, count tells."""
        R, E = self.R, self.E

        def call(cap, *ptrs):
            self._check(self.lib.sg_road_info(self.h, cap, *ptrs, int(bool(torch_out))), "sg_road_info")

        if torch_out:
            (count, geoms, layers), (p_count, p_geoms, p_layers) = self._outputs(
                True, ((R, E), "int32", "int32"), ((R, E, int(cap)), "int32", "int32"), ((R, E), "uint32", "int32"))
            call(int(cap), p_count, p_geoms, p_layers)
            self._check(self.lib.sg_synchronize(self.h), "sg_synchronize")
            return count, geoms, layers
        return self._road_query((R, E), cap, call)

    def _road_query(self, shape, cap, call):
        """(count [shape], geoms [shape, cap], layers [shape]) as numpy arrays filled by call(cap, count, geoms, layers -- their
        addresses); asked once more with cap = count.max() when some list did not fit."""
        cap = int(cap)
        while True:
            (count, geoms, layers), (_, p_geoms, _) = self._outputs(False, (shape, "int32", "int32"), (shape + (cap,), "int32", "int32"), (shape, "uint32", "int32"))
            call(cap, count.ctypes.data, p_geoms, layers.ctypes.data)  # (count is never null: no points is a valid question)
            if count.size == 0 or int(count.max()) <= cap:
                return count, geoms, layers
            cap = int(count.max())

    def road_info_points(self, scenario_of_point, xy, cap=32):
        """RoadNetwork.get_geometries_at_point (road_network/road_network.py:375-407) for n points (sg_road_info_points):
        point k = xy[k] against the network of scenario scenario_of_point[k].  Returns (count [n], geoms [n, cap], layers [n])
        as road_info does, re-queried once when a list would not fit."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        scen = np.ascontiguousarray(np.broadcast_to(np.asarray(scenario_of_point, np.int32), (len(xy),)))

        def call(cap, *ptrs):
            self._check(self.lib.sg_road_info_points(self.h, len(xy), scen.ctypes.data, xy.ctypes.data, cap, *ptrs), "sg_road_info_points")

        return self._road_query((len(xy),), cap, call)

    def set_observers(self, scenario, slot):
        """sg_set_observers: the observers of every `*_observers` call and of route_observation(observers=True) (the rows of
        obs_table.KINDS) -- observer k is entity slot
        slot[k] of scenario scenario[k], any entity of its scenario (the reference builds its sensors per entity:
        sensor/map.py:136-271, sensor/common.py:60-106).  Duplicates and any order are fine; an empty list clears it; upload()
        forgets it.  A refused list (index out of range, a slot without an entity) leaves the engine without observers."""
        _keep, n, p_scen, p_slot = self._entity_list(scenario, slot, "set_observers")
        self._n_obs = 0
        self._check(self.lib.sg_set_observers(self.h, n, p_scen, p_slot), "sg_set_observers")
        self._n_obs = n

    def raster_map_observers(self, layers, width=20.0, height=20.0, nw=20, nh=20, torch_out=False):
        """RasterizedMapSensor._step (sensor/map.py:136-271) in the frame of every observer of set_observers
        (sg_raster_map_observers): bool [n, n_layers, nh, nw]; layers as in raster_map.  An observer that is not in the scene
        gets zeros.  torch_out: a torch uint8 tensor in HBM the kernel writes directly; this wrapper waits for the kernel
        (sg_synchronize) before it returns, so the tensor can be used on any torch stream -- the C call itself does not wait."""
        (out,) = self._observation("raster", True, (layers, width, height, nw, nh), torch_out)
        return out if torch_out else out.astype(bool)

    def raster_map_observers_queued(self, out, layers, width=20.0, height=20.0, nw=20, nh=20, ordered=True):
        """raster_map_observers into `out`, a contiguous torch uint8 tensor [n, n_layers, nh, nw] on this GPU, without any host
        wait: the kernel is queued on the engine's stream behind the work of torch's current stream, and torch's current stream
        is ordered behind it (ordered=False: the caller orders the two streams itself, ordered_with_torch).  Returns `out`."""
        return self._observation("raster", True, (layers, width, height, nw, nh), into=(out,), ordered=ordered)[0]

    def future_collision_observers(self, horizon=5.0, n_samples=10, torch_out=False):
        """FutureCollisionDetector._step (sensor/common.py:87-106) for every observer of set_observers at the current time of
        its scenario (sg_future_collision_observers): bool [n], or with torch_out a torch uint8 tensor in HBM (waited for, as
        in raster_map_observers)."""
        (out,) = self._observation("future", True, (horizon, n_samples), torch_out)
        return out if torch_out else out.astype(bool)

    def nearest_entities(self, k, radius=float("inf"), torch_out=False):
        """The vector observation of the ego of every scenario (sg_nearest_entities): the k <= 32 nearest other entities that are
        in the scene and within `radius` of the ego (inclusive), by ascending (squared distance, slot).  Returns (feat [R, k, 8]
        float64, slots [R, k] int32, count [R] int32): per neighbour the longitudinal and lateral offset in the ego's frame, cos
        and sin of the relative heading, the relative velocity in that frame, box length and width; slots -1 and features 0
        behind the last neighbour; count = the candidates within the radius (it may exceed k), -1 for an ego that is not in the
        scene.  torch_out: torch tensors in HBM the kernel writes directly (waited for, as in raster_map_observers)."""
        return self._observation("nearest", False, (k, radius), torch_out)

    def nearest_entities_observers(self, k, radius=float("inf"), torch_out=False):
        """nearest_entities for every observer of set_observers (sg_nearest_entities_observers): (feat [n, k, 8], slots [n, k],
        count [n]); empty arrays when no observers are set."""
        return self._observation("nearest", True, (k, radius), torch_out)

    def pose_history(self, n_samples, stride=1, k=0, radius=float("inf"), torch_out=False):
        """The pose history of the ego of every scenario (sg_pose_history): where the ego and its k <= 32 nearest entities --
        those nearest_entities(k, radius) selects at the current state, in its order -- were at the last n_samples <= 64 rows of
        the pose record, `stride` rows apart, in the ego's current frame.  Returns (feat [R, 1 + k, n_samples, 6] float64, slots
        [R, k] int32, count [R] int32): feat[:, 0] is the ego's own history, feat[:, i] neighbour i's; sample 0 is the current
        state, sample j the record row j * stride steps back; per sample the longitudinal and lateral offset in the ego's
        frame now, cos and sin of the heading then relative to the ego's now, the age of the sample in seconds, and 1.0 -- or
        six zeros for a sample from before the episode began, for an entity that was not in the scene then, and behind the last
        neighbour.  count = the candidates within the radius, -1 (and zeros) for an ego that is not in the scene, -2 (and
        zeros) when the scenario's record filled up and it went on stepping.  Needs an engine created with record_capacity > 0
        that covers the episode: the record takes record_capacity * 6 * R * EP * 8 bytes of device memory (EP: E rounded up to
        64), and snapshots copy it.  Every kind of reset starts the history anew.  torch_out: torch tensors in HBM the kernel
        writes directly (waited for, as in raster_map_observers)."""
        return self._observation("pose_history", False, (n_samples, stride, k, radius), torch_out)

    def pose_history_observers(self, n_samples, stride=1, k=0, radius=float("inf"), torch_out=False):
        """pose_history for every observer of set_observers (sg_pose_history_observers): (feat [n, 1 + k, n_samples, 6], slots
        [n, k], count [n]); empty arrays when no observers are set."""
        return self._observation("pose_history", True, (n_samples, stride, k, radius), torch_out)

    def pose_history_observers_queued(self, feat, slots, count, stride=1, radius=float("inf"), ordered=True):
        """pose_history_observers into `feat` [n, 1 + k, n_samples, 6] float64, `slots` [n, k] int32 and `count` [n] int32,
        contiguous torch tensors on this GPU (k and n_samples are read off feat), without any host wait: the kernel is queued on
        the engine's stream behind the work of torch's current stream, and torch's current stream is ordered behind it
        (ordered=False: the caller orders the two streams itself, ordered_with_torch).  Returns (feat, slots, count)."""
        return self._observation("pose_history", True, (feat.shape[2], stride, feat.shape[1] - 1, radius), into=(feat, slots, count), ordered=ordered)

    def set_lanes(self, networks):
        """sg_set_lanes: the lane centre lines of the networks of set_road_networks, which comes first (its net_of_scenario
        holds).  networks: one lane_arrays() dict (pt_off, pts, succ_off, succ; scenario_gym_amd.road_network.RoadNetwork) per
        network of that call, in its order.  Needed by lane_observation; upload() and set_road_networks() forget the lanes."""
        lane_off, pt_off, succ_off, pts, succ = [0], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [], []
        n_pts = n_succ = 0
        for a in networks:
            po, so = np.asarray(a["pt_off"], np.int64), np.asarray(a["succ_off"], np.int64)
            pt_off.append(po[1:] + n_pts)  # (running totals: a network without lanes adds nothing)
            succ_off.append(so[1:] + n_succ)
            n_pts, n_succ = n_pts + int(po[-1]), n_succ + int(so[-1])
            pts.append(np.asarray(a["pts"], np.float64).reshape(-1, 2))
            succ.append(np.asarray(a["succ"], np.int32).ravel())
            lane_off.append(lane_off[-1] + len(po) - 1)
        lane_off = np.array(lane_off, np.int64)
        pt_off, succ_off = np.concatenate(pt_off), np.concatenate(succ_off)
        pts = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2)))
        succ = np.ascontiguousarray(np.concatenate(succ) if succ else np.zeros(0, np.int32))
        p = lambda a: a.ctypes.data  # noqa: E731
        st = L.SgLanes(len(networks), p(lane_off), p(pt_off), p(pts), p(succ_off), p(succ))
        self._check(self.lib.sg_set_lanes(self.h, C.byref(st)), "sg_set_lanes")

    def lane_observation(self, k=3, n_ahead=4, spacing=2.0, radius=float("inf"), torch_out=False):
        """The lane-frame vector observation of the ego of every scenario (sg_lane_observation): the k <= 8 lanes of the
        scenario's network whose centre lines are nearest to the ego and within `radius` (inclusive), by ascending (squared
        distance, lane index).  Returns (feat [R, k, 6 + 2 * n_ahead] float64, lanes [R, k] int32, count [R] int32): per lane the
        lateral offset from the centre line (left positive), cos and sin of the ego's heading relative to the lane direction,
        the arclength along the lane and what is left of it, the distance, then n_ahead <= 16 centre-line points `spacing` apart
        ahead of the ego in the ego's frame, continued through the lowest-index successors (at most four) and held at the last
        point where they end.  lanes: indices into `RoadNetwork.lanes`, -1 and zero features behind the last; count = the lanes
        within the radius (it may exceed k), -1 for an ego that is not in the scene, 0 without a network or before set_lanes.
        torch_out: torch tensors in HBM the kernel writes directly (waited for, as in raster_map_observers)."""
        return self._observation("lane", False, (k, n_ahead, spacing, radius), torch_out)

    def lane_observation_observers(self, k=3, n_ahead=4, spacing=2.0, radius=float("inf"), torch_out=False):
        """lane_observation for every observer of set_observers (sg_lane_observation_observers): (feat [n, k, 6 + 2 * n_ahead],
        lanes [n, k], count [n]); empty arrays when no observers are set."""
        return self._observation("lane", True, (k, n_ahead, spacing, radius), torch_out)

    def range_scan(self, n_rays=64, angle0=-np.pi, dangle=None, max_range=100.0, torch_out=False):
        """The range scan of the ego of every scenario (sg_range_scan): n_rays <= 1024 beams from the ego's pose point, beam b at
        the angle angle0 + b * dangle from its heading (dangle None: 2 pi / n_rays, a full turn), each against the bounding
        boxes of the other entities that are in the scene.  Returns (feat [R, n_rays, 2] float64, slots [R, n_rays] int32, hits
        [R] int32): per beam the distance to the first box it meets within max_range (inclusive; 0 from inside a box;
        max_range, which may be inf, without a hit) and the rate at which that distance changes -- the hit entity's velocity
        relative to the ego's along the beam, negative when it closes, 0 without a hit; slots: the hit entity or -1; hits: the
        beams that hit something, -1 for an ego that is not in the scene (features 0, slots -1).  torch_out: torch tensors in
        HBM the kernel writes directly (waited for, as in raster_map_observers)."""
        return self._observation("range_scan", False, (n_rays, angle0, dangle, max_range), torch_out)

    def range_scan_observers(self, n_rays=64, angle0=-np.pi, dangle=None, max_range=100.0, torch_out=False):
        """range_scan for every observer of set_observers (sg_range_scan_observers): (feat [n, n_rays, 2], slots [n, n_rays],
        hits [n]); empty arrays when no observers are set."""
        return self._observation("range_scan", True, (n_rays, angle0, dangle, max_range), torch_out)

    def surface_scan(self, layers, n_rays=64, angle0=-np.pi, dangle=None, step=0.5, n_steps=64, n_refine=16, torch_out=False):
        """The surface scan of the ego of every scenario (sg_surface_scan; set_road_networks comes first): n_rays <= 1024 beams
        from the ego's pose point, the beams of range_scan, each against the surface of every layer of `layers` (1..8 names of
        road_network.LAYER_CODES other than "entity", "impenetrable", or LAYER_* bits; duplicates are fine).  Returns (ranges
        [R, n_layers, n_rays] float64, flags [R, n_layers, n_rays] uint8, hits [R, n_layers] int32): per layer and beam the
        range at which the beam first changes side of the layer's surface -- from on it, the distance to leaving it; from off
        it, the distance to reaching it -- found by n_steps <= 4096 samples `step` apart and n_refine <= 64 bisections of the
        step that changed side (the point reported lies on the other side, the crossing at most step * 2^-n_refine before
        it; a strip narrower than `step` between two samples is stepped over), n_steps * step without a change; flags:
        SURF_HIT the beam changed side, SURF_INSIDE the pose point is on the layer; hits: the beams that changed side, -1 for
        an ego that is not in the scene (ranges and flags 0).  Without a road network every range is n_steps * step.
        torch_out: torch tensors in HBM the kernel writes directly (waited for, as in raster_map_observers)."""
        return self._observation("surface_scan", False, (layers, n_rays, angle0, dangle, step, n_steps, n_refine), torch_out)

    def surface_scan_observers(self, layers, n_rays=64, angle0=-np.pi, dangle=None, step=0.5, n_steps=64, n_refine=16, torch_out=False):
        """surface_scan for every observer of set_observers (sg_surface_scan_observers): (ranges [n, n_layers, n_rays], flags
        [n, n_layers, n_rays], hits [n, n_layers]); empty arrays when no observers are set."""
        return self._observation("surface_scan", True, (layers, n_rays, angle0, dangle, step, n_steps, n_refine), torch_out)

    def entity_status(self, torch_out=False):
        """The episode status of the ego of every scenario (sg_entity_status): what a per-agent reward and termination need in
        one launch.  Returns (flags [R] uint32, info [R, 4] int32, feat [R, 3] float64).  flags: ST_PRESENT (in the scene),
        ST_COLLISION (its State.collisions() row is not empty), ST_OFF_ROAD (ego_off_road asked of this entity: not in the scene
        or its pose point not strictly inside the driveable surface), ST_CORNER_OFF (a box corner is not), ST_HIT_VEHICLE /
        ST_HIT_PEDESTRIAN / ST_HIT_OTHER (the entity types in its row), and from bit ST_LAYER_SHIFT the LAYER_* bits of the
        polygons that contain its pose point.  info: the number of entities it collides with, the lowest of their slots (-1:
        none), how many of its four box corners are on the driveable surface, the slot of the nearest other box (-1: none).
        feat: its speed, its distance travelled, and the clearance -- the distance from its box to the nearest other box, 0
        when they collide, inf when it is alone.  An ego that is not in the scene: ST_OFF_ROAD alone, info -1, feat 0.
        torch_out: torch tensors in HBM the kernel writes directly (flags as int32 bit patterns; waited for, as in
        raster_map_observers)."""
        return self._observation("entity_status", False, (), torch_out)

    def entity_status_observers(self, torch_out=False):
        """entity_status for every observer of set_observers (sg_entity_status_observers): (flags [n], info [n, 4], feat
        [n, 3]); empty arrays when no observers are set."""
        return self._observation("entity_status", True, (), torch_out)

    def set_routes(self, scenario, slot, paths):
        """sg_set_routes: where entities are supposed to go.  Route j belongs to entity slot[j] of scenario scenario[j] (any
        entity, each at most once) and is the polyline paths[j] ([n_pts, 2], in driving order, used as given; fewer than two
        points: no segments).  Needed by the route part of route_observation; an empty list clears the routes, upload() forgets
        them, and a refused call leaves the previous ones in place."""
        if not (np.size(scenario) == np.size(slot) == len(paths)):
            raise ValueError("set_routes: one scenario, one slot and one path per route")
        _keep, n, p_scen, p_slot = self._entity_list(scenario, slot, "set_routes")
        _keep_paths, p_off, p_pts = self._path_table(paths) if n else (None, None, None)
        self._check(self.lib.sg_set_routes(self.h, n, p_scen, p_slot, p_off, p_pts), "sg_set_routes")

    def route_observation(self, n_ahead=4, spacing=2.0, observers=False, device=False):
        """The route and recorded-track observation (sg_route_observation; observers: sg_route_observation_observers, for every
        observer of set_observers instead of the ego of every scenario).  Returns (feat [n, 11 + 2 * n_ahead] float64, info
        [n, 2] int32).  feat: [0:2] where the entity's own recording has it at the current time, in the entity's frame, [2] the
        distance to it, [3:5] cos and sin of the recorded heading relative to the entity's; [5] the lateral offset from its route
        of set_routes (left positive), [6:8] cos and sin of its heading relative to the route, [8] the arclength along the
        route, [9] what is left of it, [10] the distance to it; then n_ahead <= 16 route points `spacing` apart ahead of the
        entity, in its frame, held at the route's last point.  info: the best route segment (-1: no route, or none with
        segments; features 5 and up are zero then), and where the current time lies in the recording (0 within, -1 before its
        first knot, 1 after its last).  An entity that is not in the scene: info -1, -1 and zeros.  device: torch tensors in
        HBM the kernel writes directly (waited for, as in entity_status)."""
        return self._observation("route", observers, (n_ahead, spacing), device)

    def time_to_collision(self, horizon=float("inf"), torch_out=False):
        """The time to collision of the ego of every scenario (sg_time_to_collision): when its bounding box first touches the box
        of another entity that is in the scene, within `horizon` seconds (inclusive; inf: ever), if both keep their velocity and
        heading (the yaw rate is ignored).  Returns (feat [R, 4] float64, info [R, 3] int32).  feat: the time to the first
        contact -- 0 for an entity it already collides with, inf when there is none --, the time at which that overlap ends (it
        may be inf; 0 without a contact), and the threat's velocity relative to the ego's along and across the ego's heading (0
        without).  info: the threat's slot (-1: none), the number of entities met within the horizon, and the face that meets
        first -- 0 the ego's front or rear, 1 its side, 2 / 3 the other box's front or rear / side, -1 for an overlap that exists
        already and without a threat.  An ego that is not in the scene: info -1, feat 0.  torch_out: torch tensors in HBM the
        kernel writes directly (waited for, as in entity_status)."""
        return self._observation("ttc", False, (horizon,), torch_out)

    def time_to_collision_observers(self, horizon=float("inf"), torch_out=False):
        """time_to_collision for every observer of set_observers (sg_time_to_collision_observers): (feat [n, 4], info [n, 3]);
        empty arrays when no observers are set."""
        return self._observation("ttc", True, (horizon,), torch_out)

    def time_to_collision_observers_queued(self, feat, info, horizon=float("inf"), ordered=True):
        """time_to_collision_observers into `feat` [n, 4] float64 and `info` [n, 3] int32, contiguous torch tensors on this GPU,
        without any host wait: the kernel is queued on the engine's stream behind the work of torch's current stream, and
        torch's current stream is ordered behind it (ordered=False: the caller orders the two streams itself,
        ordered_with_torch).  Returns (feat, info)."""
        return self._observation("ttc", True, (horizon,), into=(feat, info), ordered=ordered)

    def raster_map(self, layers, width=20.0, height=20.0, nw=20, nh=20):
        """RasterizedMapSensor._step (sensor/map.py:136-149) around the ego of every scenario: bool [R, n_layers, nh, nw];
        layers: 0 = entity, or one LAYER_* bit of scenario_gym_amd.road_network."""
        lay = np.ascontiguousarray(layers, np.int32)
        out = np.zeros((self.R, len(lay), int(nh), int(nw)), np.uint8)
        self._check(self.lib.sg_raster_map(self.h, float(width), float(height), int(nw), int(nh), len(lay), lay.ctypes.data,
                                           out.ctypes.data), "sg_raster_map")
        return out.astype(bool)

    def raster_map_torch(self, layers, width=20.0, height=20.0, nw=20, nh=20):
        """raster_map left on the device: a zero-copy torch uint8 view [R, n_layers, nh, nw] over the handle's observation
        scratch (valid until the next observation call), ordered after the kernels that fill it.  torch is the container."""
        key = (tuple(layers), int(nw), int(nh))
        cache = self.__dict__.setdefault("_map_views", {})
        ent = cache.get(key)
        if ent is None:
            ent = cache[key] = [np.ascontiguousarray(layers, np.int32), C.c_void_p(), None, None]
        lay, ptr = ent[0], ent[1]
        self._check(self.lib.sg_raster_map_device(self.h, float(width), float(height), key[1], key[2], len(lay), lay.ctypes.data,
                                                  C.byref(ptr)), "sg_raster_map_device")
        self._check(self.lib.sg_synchronize(self.h), "sg_synchronize")
        if ent[2] != ptr.value:  # the scratch moved (first call, or it grew): wrap the new address once
            ent[2], ent[3] = ptr.value, self._device_view(ptr.value, (self.R, len(lay), key[2], key[1]), "|u1")
        return ent[3]

    def tick(self, actions, layers, width=20.0, height=20.0, nw=20, nh=20, torch_out=False):
        """One RL tick as one graph launch (sg_tick): step(1, actions) + terminal_flags + raster_map.  actions [R, 2]: numpy,
        a float64 torch tensor on the device, or None.  Returns (obs [R, n_layers, nh, nw], flags [R]): numpy arrays (bool /
        uint32), or with torch_out zero-copy torch views (uint8 / int32) valid until the next observation call."""
        key = ("tick", tuple(layers), int(nw), int(nh))
        cache = self.__dict__.setdefault("_map_views", {})
        ent = cache.get(key)
        if ent is None:
            ent = cache[key] = [np.ascontiguousarray(layers, np.int32), C.c_void_p(), C.c_void_p(), None, None, None]
        lay, d_obs, d_fl = ent[0], ent[1], ent[2]
        _keep, ptr, on_device = self._actions(actions, 1)
        self._check(self.lib.sg_tick(self.h, ptr, on_device, float(width), float(height), key[2], key[3], len(lay),
                                     lay.ctypes.data, C.byref(d_obs), C.byref(d_fl)), "sg_tick")
        self._check(self.lib.sg_synchronize(self.h), "sg_synchronize")
        shape = (self.R, len(lay), key[3], key[2])
        if not torch_out:
            obs, fl = np.empty(shape, np.uint8), np.empty(self.R, np.uint32)
            self._check(self.lib.sg_copy_to_host(self.h, d_obs, obs.ctypes.data, obs.nbytes), "sg_copy_to_host")
            self._check(self.lib.sg_copy_to_host(self.h, d_fl, fl.ctypes.data, fl.nbytes), "sg_copy_to_host")
            return obs.astype(bool), fl
        if ent[3] != (d_obs.value, d_fl.value):
            ent[3] = (d_obs.value, d_fl.value)
            ent[4], ent[5] = self._device_view(d_obs.value, shape, "|u1"), self._device_view(d_fl.value, (self.R,), "<i4")
        return ent[4], ent[5]

    def rollout(self, max_steps):
        self._check(self.lib.sg_rollout(self.h, int(max_steps)), "sg_rollout")

    def rollout_async(self, max_steps, do_reset=True):
        self._check(self.lib.sg_rollout_async(self.h, int(max_steps), int(do_reset)), "sg_rollout_async")

    def synchronize(self):
        self._check(self.lib.sg_synchronize(self.h), "sg_synchronize")

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(self.lib.sg_last_kernel_ms(self.h, C.byref(ms)), "sg_last_kernel_ms")
        return ms.value

    def set_tuning(self, tab_min_steps=-1, chunk_steps=0, overlap=-1):
        """Launch policy (sg_set_tuning); results never depend on it."""
        self._check(self.lib.sg_set_tuning(self.h, int(tab_min_steps), int(chunk_steps), int(overlap)), "sg_set_tuning")

    def set_slicing(self, on=True):
        """sg_set_slicing: may sg_rollout cut the time axis of a small replay-only batch into slices (results never depend on
        it; the intermediate states are not written to memory when it does)."""
        self._check(self.lib.sg_set_slicing(self.h, 2 if on == "always" else int(bool(on))), "sg_set_slicing")

    def last_launch_stats(self):
        """(number of rollout-kernel launches of the last call, the time in ms during which at least one of them ran)."""
        n, ms = C.c_int32(), C.c_float()
        self._check(self.lib.sg_last_launch_stats(self.h, C.byref(n), C.byref(ms)), "sg_last_launch_stats")
        return n.value, ms.value

    def last_launch_gross_ms(self):
        """Sum of the durations of those launches (launches of the two pipelines overlap: more than the time above)."""
        ms = C.c_float()
        self._check(self.lib.sg_last_launch_gross_ms(self.h, C.byref(ms)), "sg_last_launch_gross_ms")
        return ms.value

    def schedule_info(self):
        """The launch schedule of the last rollout / step call (sg_schedule_info): schedule 0 = not the table path, 1 = chunk
        launches, 2 = one persistent launch (csrc/sgym_queue.hpp); its chunks, table-ring buffers and wavefronts; the
        pre-pass wavefronts, blocks and SIMDs; the rollout-kernel launches of the call."""
        v = (C.c_int32 * 8)()
        self._check(self.lib.sg_schedule_info(self.h, v), "sg_schedule_info")
        return dict(schedule=v[0], chunks=v[1], ring=v[2], grid=v[3], ctl_waves=v[4], blocks=v[5], simds=v[6], launches=v[7])

    def last_kernel(self):
        """The rollout entry point the handle launched last (sg_last_kernel), e.g. "sg::rollout_kernel_crowd<4>"."""
        return (self.lib.sg_last_kernel(self.h) or b"").decode()

    def debug_trig32(self, heading):
        """The broad phase's fp32 (sin, cos) of fp64 headings (test hook)."""
        h = np.ascontiguousarray(heading, np.float64).ravel()
        s, c = np.empty(h.size, np.float32), np.empty(h.size, np.float32)
        self._check(self.lib.sg_debug_trig32(self.h, h.size, h.ctypes.data, s.ctypes.data, c.ctypes.data),
                    "sg_debug_trig32")
        return s, c

    # ------------------------------------------------------------------ reads
    def _d2h(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        self._check(self.lib.sg_copy_to_host(self.h, ptr, out.ctypes.data, out.nbytes), "sg_copy_to_host")
        return out

    def state(self, raw=False):
        """Host copy of the step-materialised state: dict of [R, E, ...] arrays (NaN = absent).
        `coll` is [R, E] uint64 for up to 64 entities, else [R, E, row_words].
        raw: the stored pose / velocity rows as they are, also for entities that are not in the scene (debugging, tests)."""
        v, R, E, EP = self._view, self.R, self.E, self._view.entity_stride
        n = R * EP
        blocks = self._d2h(v.blocks, (v.n_blocks, v.block_rows, 64), np.float64)

        def rows(f, k=1, dtype=np.float64):
            a = blocks[:, f:f + k, :].view(dtype)                      # [nblk, k, 64]
            return np.moveaxis(a, 1, -1).reshape(-1, k)[:n].reshape(R, EP, k)[:, :E]

        present = rows(L.F_PRESENT, 1, np.uint64)[..., 0] != 0
        scen = self._d2h(v.scen, R, SCEN_DTYPE)
        coll = rows(L.F_COLL, v.row_words, np.uint64)
        return dict(
            poses=rows(L.F_POSE, 6).copy() if raw else np.where(present[..., None], rows(L.F_POSE, 6), np.nan),
            vels=rows(L.F_VEL, 6).copy() if raw else np.where(present[..., None], rows(L.F_VEL, 6), np.nan),
            present=present, dists=rows(L.F_DIST)[..., 0], coll=coll[..., 0] if v.row_words == 1 else coll,
            ctrl_state=rows(L.F_CTRL, 4), force=rows(L.F_FORCE, 2), t=scen["t"].copy(), prev_t=scen["prev_t"].copy(),
            done=scen["done"].astype(bool), n_steps=scen["n_steps"].copy(), noise_pos=scen["noise_pos"].copy(),
            rec_rows=scen["rec_rows"].copy(),
        )

    METRIC_DTYPE = np.dtype([("ego_avg_speed", "f8"), ("ego_max_speed", "f8"), ("ego_distance_travelled", "f8"),
                             ("final_t", "f8"), ("n_steps", "i4"), ("done", "i4"), ("n_collisions", "i4"), ("reserved", "i4")])
    EVENT_DTYPE = np.dtype([("t", "f8"), ("scenario", "i4"), ("other", "i4"), ("type", "i4"), ("reserved", "i4")])

    def metrics(self, event_cap=None):
        """(per-scenario metric rows, CollisionMetric events) as structured arrays (sg_metrics / sg_event layout)."""
        cap = self.R * max(self.cfg.event_capacity, 1) if event_cap is None else int(event_cap)
        rows = np.empty(self.R, self.METRIC_DTYPE)   # uninitialised host buffers: the library fills what it reports
        if getattr(self, "_ev_buf", None) is None or len(self._ev_buf) < cap:
            self._ev_buf = np.empty(cap, self.EVENT_DTYPE)   # kept between calls (6 MB for 4096 x 64: not touched unless filled)
        ev = self._ev_buf
        n_ev = C.c_int32()
        self._check(self.lib.sg_read_metrics(self.h, rows.ctypes.data_as(C.POINTER(L.SgMetrics)),
                                             ev.ctypes.data_as(C.POINTER(L.SgEvent)), cap, C.byref(n_ev)), "sg_read_metrics")
        return rows, ev[: n_ev.value].copy()

    def set_rss(self, enabled=True):
        """reset / rollout / step run the RSSDistances callback themselves after the reset and after every step."""
        self._check(self.lib.sg_set_rss(self.h, int(bool(enabled))), "sg_set_rss")

    def rss_update(self, reset=False):
        """RSSDistances.__call__ on the current state of every scenario (after a reset: reset=True)."""
        self._check(self.lib.sg_rss_update(self.h, int(bool(reset))), "sg_rss_update")

    def rss(self):
        """(safe_longitudinal [R] bool, safe_lateral [R] bool, codes [R, E], safe distances [R, E, 2]) of the RSS callback."""
        flags = np.zeros(self.R, np.uint8)
        codes = np.zeros((self.R, self.E), np.int32)
        safe = np.zeros((self.R, self.E, 2))
        self._check(self.lib.sg_rss_read(self.h, flags.ctypes.data, codes.ctypes.data, safe.ctypes.data), "sg_rss_read")
        return (flags & 1) != 0, (flags & 2) != 0, codes, safe

    def collision_points(self, event_cap=None):
        """CollisionPointMetric for the events of metrics(), same order: [n_events, 3] = x, y, relative heading."""
        cap = int(event_cap or self.R * max(int(self.cfg.event_capacity), 1))
        out = np.empty((cap, 3))
        n = C.c_int32()
        self._check(self.lib.sg_read_collision_points(self.h, out.ctypes.data, cap, C.byref(n)), "sg_read_collision_points")
        return out[: n.value].copy()

    def record(self, n_rows):
        """State.recorded_poses for the whole batch: t [n, R], poses [n, R, E, 6]."""
        t = np.empty((n_rows, self.R))
        poses = np.empty((n_rows, self.R, self.E, 6))
        self._check(self.lib.sg_read_record(self.h, int(n_rows), t.ctypes.data, poses.ctypes.data), "sg_read_record")
        return t, poses

    def torch_state(self):
        """Zero-copy torch view [n_blocks, block_rows, 64] (fp64) over the device state blocks;
        field f of entity i is view[i // 64, f, i % 64].  torch is only the container."""
        v = self._view
        return self._device_view(v.blocks, (v.n_blocks, v.block_rows, 64), "<f8")

