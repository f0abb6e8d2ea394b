"""The observation kinds of the engine, one row each: which C pair serves a kind, how the caller's arguments are cast for it, what
it writes, and what must be on the device first.  RolloutEngine._observation runs every kind from its row; BatchedScenarioGym
and VectorScenarioEnv take the public method names and the prerequisites from it.  A new kind is one row here, one line in
_lib.OBSERVATION_ARGTYPES and its public methods with their docstrings ("Adding an observation")."""
from collections import namedtuple

import numpy as np

from . import _lib as L

# stem: the C pair sg_<stem> / sg_<stem>_observers (ego_c False: sg_<stem> has another signature and is not called from here).
# ego, observers: RolloutEngine's public methods (one name twice: the method takes observers=True).
# args(*user arguments -- all of them: the defaults are the public methods') -> (the C arguments between the handle and the
#   outputs, what must stay alive across the call).
# outs(n, *C arguments) -> ((shape, numpy dtype, torch dtype), ...) of the outputs for n egos / observers, in the C call's order.
# needs: what must be on the device first, of "roads", "lanes" (behind the roads), "routes", "record".
# torch_kw: the keyword of the public methods that asks for torch tensors in HBM.
Kind = namedtuple("Kind", "stem ego observers args outs needs ego_c torch_kw", defaults=((), True, "torch_out"))

F8, I4, U1 = ("float64", "float64"), ("int32", "int32"), ("uint8", "uint8")


def _dangle(n_rays, dangle):
    return 2.0 * np.pi / max(n_rays, 1) if dangle is None else float(dangle)  # (n_rays < 1 is the library's to refuse)


def _raster_args(layers, width, height, nw, nh):
    lay = np.ascontiguousarray(layers, np.int32)
    return (float(width), float(height), int(nw), int(nh), len(lay), lay.ctypes.data), lay


def _surface_args(layers, n_rays, angle0, dangle, step, n_steps, n_refine):
    from .road_network import surface_layer_bits

    lay = np.ascontiguousarray(surface_layer_bits(layers), np.int32)
    n_rays = int(n_rays)
    return (len(lay), lay.ctypes.data if len(lay) else None, n_rays, float(angle0), _dangle(n_rays, dangle), float(step), int(n_steps),
            int(n_refine)), lay


def _surface_outs(n, nl, _lay, n_rays, *_):
    cells = (n, nl, max(n_rays, 0))
    return (cells, *F8), (cells, *U1), ((n, nl), *I4)


def _range_args(n_rays, angle0, dangle, max_range):
    n_rays = int(n_rays)
    return (n_rays, float(angle0), _dangle(n_rays, dangle), float(max_range)), None


KINDS = {
    "raster": Kind("raster_map", "raster_map", "raster_map_observers", _raster_args,
                   lambda n, w, h, nw, nh, nl, _lay: (((n, nl, nh, nw), *U1),), ego_c=False),  # (roads for a surface layer: the caller's to tell)
    "future": Kind("future_collision", "future_collision", "future_collision_observers",
                   lambda horizon, n_samples: ((float(horizon), int(n_samples)), None),
                   lambda n, *_: (((n,), *U1),), ego_c=False),
    "nearest": Kind("nearest_entities", "nearest_entities", "nearest_entities_observers",
                    lambda k, radius: ((int(k), float(radius)), None),
                    lambda n, k, _r: (((n, k, 8), *F8), ((n, k), *I4), ((n,), *I4))),
    "pose_history": Kind("pose_history", "pose_history", "pose_history_observers",
                         lambda n_samples, stride, k, radius: ((int(n_samples), int(stride), int(k), float(radius)), None),
                         lambda n, H, _s, k, _r: (((n, 1 + max(k, 0), max(H, 0), L.HIST_NFEAT), *F8), ((n, max(k, 0)), *I4), ((n,), *I4)),
                         needs=("record",)),
    "lane": Kind("lane_observation", "lane_observation", "lane_observation_observers",
                 lambda k, n_ahead, spacing, radius: ((int(k), int(n_ahead), float(spacing), float(radius)), None),
                 lambda n, k, n_ahead, *_: (((n, k, 6 + 2 * max(n_ahead, 0)), *F8), ((n, k), *I4), ((n,), *I4)), needs=("lanes",)),
    "range_scan": Kind("range_scan", "range_scan", "range_scan_observers", _range_args,
                       lambda n, n_rays, *_: (((n, max(n_rays, 0), 2), *F8), ((n, max(n_rays, 0)), *I4), ((n,), *I4))),
    "surface_scan": Kind("surface_scan", "surface_scan", "surface_scan_observers", _surface_args, _surface_outs, needs=("roads",)),
    # (the flag word: uint32 on the host; torch has no such type on every build, so the tensor holds the int32 bit patterns)
    "entity_status": Kind("entity_status", "entity_status", "entity_status_observers", lambda: ((), None),
                          lambda n: (((n,), "uint32", "int32"), ((n, L.ST_NINFO), *I4), ((n, L.ST_NFEAT), *F8)), needs=("roads",)),
    "route": Kind("route_observation", "route_observation", "route_observation",
                  lambda n_ahead, spacing: ((int(n_ahead), float(spacing)), None),
                  lambda n, n_ahead, _s: (((n, L.RT_NFEAT + 2 * max(n_ahead, 0)), *F8), ((n, L.RT_NINFO), *I4)),
                  needs=("routes",), torch_kw="device"),
    "ttc": Kind("time_to_collision", "time_to_collision", "time_to_collision_observers",
                lambda horizon: ((float(horizon),), None),
                lambda n, _h: (((n, L.TTC_NFEAT), *F8), ((n, L.TTC_NINFO), *I4))),
}


def public_call(engine, kind, observers, args, torch_out=None):
    """`kind` for the egos or the observers through the engine's public method of that name (a stand-in engine needs only
    those); torch_out None: the keyword is left out."""
    row = KINDS[kind]
    kw = {"observers": True} if observers and row.observers == row.ego else {}
    if torch_out is not None:
        kw[row.torch_kw] = torch_out
    return getattr(engine, row.observers if observers else row.ego)(*args, **kw)


def blank(kind, lead, fills, *args):
    """One numpy array per output of `kind`, a row per cell of `lead` in place of a row per observer, filled with fills[j]."""
    specs = KINDS[kind].outs(0, *KINDS[kind].args(*args)[0])
    return tuple(np.full(tuple(lead) + shape[1:], fill, dt) for (shape, dt, _), fill in zip(specs, fills))
