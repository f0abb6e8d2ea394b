#!/usr/bin/env python3
"""Golden vectors for the pedestrian route finder (pedestrian/route.py) from the REAL reference: tests/golden/route.npz.

    SG_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_route.py

The reference's RouteFinder on the Greenwich network (Road_Networks/Greenwich_Road_Network_002.json of its test inputs, also
in inputs_roads_1.npz: 5 pavements, 4 crossings), imported with the stand-ins of tests/golden/_refstubs (the centre-line
interpolation it calls is the stand-in's): the connection graph, its node indices and positions, and the breadth-first routes
between 12 pairs of seeded random points.  Only data is written: the query points and the reference's answers, as one JSON
string."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SG_REFERENCE")
if not REF:
    raise SystemExit("make_golden_route: set SG_REFERENCE to a checkout of the reference")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path[:0] = [os.path.join(HERE, "_refstubs"), REF]

import numpy as np  # noqa: E402

from scenario_gym.pedestrian.route import RouteFinder  # noqa: E402
from scenario_gym.road_network import RoadNetwork  # noqa: E402

NETWORK = "Greenwich_Road_Network_002"


def queries():
    """12 (start, goal) pairs, uniform over the network's extent (the consumer's own copy of them is in the file)."""
    rng = np.random.default_rng(0)
    lo, hi = np.array([290.0, 288.0]), np.array([591.0, 496.0])
    return rng.uniform(lo, hi, (12, 2, 2))


def main():
    rf = RouteFinder(RoadNetwork.create_from_json(os.path.join(REF, "tests", "input_files", "Road_Networks", NETWORK + ".json")))
    q = queries()
    routes = [rf.find_route(a, b) for a, b in q]
    res = dict(graph={str(k): v for k, v in rf.graph.items()}, idx=rf.node_to_idx,
               data={str(k): list(map(float, v)) for k, v in rf.node_data.items()},
               routes=[None if r is None else np.asarray(r).tolist() for r in routes])
    np.savez_compressed(os.path.join(os.environ.get("SG_GOLDEN_OUT", HERE), "route.npz"), network=np.array(NETWORK), queries=q,
                        result=np.array(json.dumps(res, sort_keys=True)))


if __name__ == "__main__":
    main()
