"""The scenes of tests/box_scenes.py on the CPU: before the device is compared with the oracle on them
(tests/test_gpu_boxes.py), the oracle is compared with the exact answer, and the scenes are shown to hold what they are for.

* On every scenario of every scene the GPU tests use, after every step they check, sgo_quads_intersect on the oracle's
  corners equals the exact answer for EVERY pair whose bounding circles touch.  No pair, no step and no scenario is left out
  and there is no band: the poses are continuous random draws, so fp64 and the exact answer differ only for a pair within
  rounding of touching, and no seed here produces one.  HOW the exact answer is had: box_scenes.exact_pairs puts an fp64
  separating-axis filter in front of the rational arithmetic (_decided_in_fp64: a gap counts as decided only beyond 1e-9 x
  the magnitudes, five orders above its rounding error; it is checked against the 10,000 exact labels of collision.npz
  below), and quads_meet_exact -- the SAT in fractions.Fraction -- runs only for the pairs inside that margin and for every
  pair with a zero-extent box (a zero edge decides nothing in fp64).  This is NOT a Fraction SAT of every pair; the printed
  tallies say how many pairs it was.
* Every scene has DECISIVE pair-steps: pairs whose exact answer flips when center_y is dropped, when the whole centre offset is
  dropped, when width and length are swapped, when the giant is shrunk to the scene's median box -- in both directions, a
  collision lost and a collision invented.  Those are the pairs a device kernel with one of these mistakes gets wrong.
  MIN_DECISIVE holds half of what the generator yields.  For the shrunk giant some decisive pair crosses a wavefront boundary
  (scenarios of more than 64 slots) and a 256-slot tile boundary (more than 512).
"""
import numpy as np
import pytest

import box_scenes as B
from conftest import load_golden

# (recipe, entity slots, ego, far): every batch tests/test_gpu_boxes.py uploads (its test_scenes_are_checked_on_the_cpu)
SCENES = ([("yard", E, "sparse", False) for E in (3, 6, 12, 24, 48, 100, 200, 300, 600, 1100)]
          + [("yard", E, "replay", False) for E in (6, 24, 48)]
          + [("mixed", E, "sparse", False) for E in (12, 48, 100, 200, 300, 600)]
          + [("yard", 12, "sparse", True), ("yard", 100, "sparse", True), ("mixed", 12, "sparse", True),
             ("mixed", 100, "sparse", True)])


def scene_id(s):
    return f"{s[0]}-E{s[1]}-{s[2]}" + ("-far" if s[3] else "")


# per scene: (lost, invented) pair-steps per modification of box_scenes.MODS, half of what the generator yields (rounded down)
MIN_DECISIVE = {
    "yard-E3-sparse": [[60, 72], [49, 115], [107, 56], [95, 49]],
    "yard-E6-sparse": [[120, 118], [186, 244], [213, 132], [209, 45]],
    "yard-E12-sparse": [[266, 184], [374, 295], [443, 264], [386, 22]],
    "yard-E24-sparse": [[282, 331], [454, 593], [511, 432], [328, 66]],
    "yard-E48-sparse": [[318, 417], [614, 903], [690, 573], [318, 54]],
    "yard-E100-sparse": [[553, 658], [1088, 1427], [1183, 1030], [316, 11]],
    "yard-E200-sparse": [[1250, 1177], [2473, 2351], [2164, 1843], [489, 27]],
    "yard-E300-sparse": [[1256, 1374], [2695, 2819], [2170, 2062], [348, 63]],
    "yard-E600-sparse": [[1350, 1256], [2774, 2708], [2177, 2118], [179, 27]],
    "yard-E1100-sparse": [[1231, 1159], [2614, 2637], [1847, 1846], [109, 31]],
    "yard-E6-replay": [[126, 126], [187, 253], [214, 139], [210, 45]],
    "yard-E24-replay": [[291, 346], [469, 612], [528, 443], [336, 66]],
    "yard-E48-replay": [[322, 417], [617, 903], [691, 569], [318, 54]],
    "mixed-E12-sparse": [[208, 334], [283, 512], [383, 321], [323, 93]],
    "mixed-E48-sparse": [[457, 563], [746, 1055], [792, 789], [428, 101]],
    "mixed-E100-sparse": [[870, 931], [1503, 1813], [1595, 1344], [578, 34]],
    "mixed-E200-sparse": [[1339, 1493], [2968, 3109], [2493, 2201], [640, 56]],
    "mixed-E300-sparse": [[1502, 1503], [3139, 3251], [2547, 2445], [386, 48]],
    "mixed-E600-sparse": [[1355, 1558], [3086, 3389], [2434, 2359], [269, 25]],
    "yard-E12-sparse-far": [[202, 148], [269, 229], [318, 194], [291, 20]],
    "yard-E100-sparse-far": [[850, 1015], [1721, 2053], [1743, 1486], [467, 21]],
    "mixed-E12-sparse-far": [[179, 255], [241, 385], [336, 235], [272, 57]],
    "mixed-E100-sparse-far": [[1188, 1274], [2069, 2460], [2147, 1824], [823, 41]],
}


def _tally(oracle, scene):
    """(near pair-steps, colliding ones, disagreements oracle / exact, [4][2] decisive tallies, decisive pairs of the shrunk
    giant that cross a wavefront / a 256-slot tile boundary, pairs that needed the rational arithmetic)."""
    recipe, E, ego, far = scene
    steps = B.steps_of(E)
    near = hits = 0
    bad = []
    tally = np.zeros((len(B.MODS), 2), int)
    cross64 = cross256 = 0
    n0 = B.N_RATIONAL[0]
    for r, sc in enumerate(B.batch(recipe, E, ego, far)):
        o = B.oracle_rollout(oracle, sc, steps)
        assert o["n_steps"] == steps and not o["is_done"]
        poses = o["poses"][1:]  # the states after steps 1 .. steps
        key = scene + (r,)
        cor = B.corners_table(oracle.corners, poses, sc["bbox"])
        for (k, i, j), hit in B.exact_pairs(key, cor).items():
            near += 1
            hits += hit
            if oracle.quads_intersect(cor[k, i], cor[k, j]) != hit or oracle.quads_intersect(cor[k, j], cor[k, i]) != hit:
                bad.append((r, k + 1, i, j))
        g = B.giant_slot(sc["bbox"])
        assert g == sc["giant"] and (g == E - 1 or E <= 64)
        for m, mod in enumerate(B.MODS):
            lost, invented = B.decisive_pairs(key, oracle.corners, poses, sc["bbox"], mod)
            tally[m] += (len(lost), len(invented))
            if m == 3:
                assert all(g in p[1:] for p in lost + invented)
                cross64 += sum((p[1] >> 6) != (p[2] >> 6) for p in lost + invented)
                cross256 += sum((p[1] >> 8) != (p[2] >> 8) for p in lost + invented)
    return near, hits, bad, tally, cross64, cross256, B.N_RATIONAL[0] - n0


@pytest.mark.parametrize("scene", SCENES, ids=[scene_id(s) for s in SCENES])
def test_oracle_is_exact_on_the_scene_and_the_scene_is_decisive(oracle, scene):
    """The two bullet points of the module docstring for one scene."""
    E = scene[1]
    near, hits, bad, tally, cross64, cross256, rational = _tally(oracle, scene)
    print(f"{scene_id(scene)}: {near} near pair-steps, {hits} meet, {rational} decided by rational arithmetic; decisive "
          f"(lost, invented) {dict(zip(B.MODS, tally.tolist()))}; shrunk giant across wavefronts {cross64}, across tiles {cross256}")
    assert not bad, bad[:10]  # (scenario, step, i, j): NO pair is excluded
    assert 2 * hits > B.steps_of(E) * len(B.batch(*scene))  # (dense: on average a collision every other step, at least)
    want = np.array(MIN_DECISIVE[scene_id(scene)])
    assert (want >= 1).all() and (tally >= want).all(), (tally.tolist(), want.tolist())
    if E > 64:
        assert cross64 >= 1
    if E > 512:
        assert cross256 >= 1


def test_exact_predicate_reproduces_the_labelled_pairs():
    """quads_meet_exact and the fp64 filter in front of it against the 10,000 pairs of collision.npz, labelled by exact
    rational SAT when the fixture was made (other code, the reference's corners): every label, and the filter is never wrong
    where it claims to know."""
    g = load_golden("collision")
    lab = g["pairs/intersects"].astype(bool)
    A, Bq = g["pairs/corners_a"], g["pairs/corners_b"]
    assert np.array_equal(np.array([B.quads_meet_exact(a, b) for a, b in zip(A, Bq)]), lab)
    apart, meet = B._decided_in_fp64(A, Bq)
    assert not (apart & lab).any() and not (meet & ~lab).any() and (apart | meet).mean() > 0.99


def test_exact_predicate_on_touching_and_flat_quads():
    """Closed sets: a shared edge, a shared corner and containment meet; one ulp of daylight does not; zero-extent boxes
    (segments) are decided too -- crossing, touching at an end point, collinear and apart, collinear and overlapping."""
    sq = lambda x, y, w=1.0, h=1.0: np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]])  # noqa: E731
    assert B.quads_meet_exact(sq(0, 0), sq(1, 0)) and B.quads_meet_exact(sq(0, 0), sq(1, 1))
    assert B.quads_meet_exact(sq(0, 0, 4, 4), sq(1, 1)) and B.quads_meet_exact(sq(0, 0), sq(0, 0)[::-1])
    assert not B.quads_meet_exact(sq(0, 0), sq(np.nextafter(1.0, 2.0), 0))
    assert not B.quads_meet_exact(sq(0, 0), sq(np.nextafter(1.0, 2.0), np.nextafter(1.0, 2.0)))
    seg = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y1], [x1, y1], [x0, y0]], float)  # noqa: E731
    assert B.quads_meet_exact(seg(0, 0, 2, 2), seg(0, 2, 2, 0)) and B.quads_meet_exact(seg(0, 0, 1, 0), seg(1, 0, 1, 5))
    assert not B.quads_meet_exact(seg(0, 0, 1, 0), seg(2, 0, 3, 0)) and B.quads_meet_exact(seg(0, 0, 2, 0), seg(1, 0, 3, 0))
    assert B.quads_meet_exact(seg(0.5, -1, 0.5, 1), sq(0, 0)) and not B.quads_meet_exact(seg(2, -1, 2, 1), sq(0, 0))
    for box in B.ZERO_EXTENT:  # (what such a box is: a quad without area)
        assert B._area2(B._ints(B.corners_numpy(np.array([1.0, 2.0, 0.0, 0.7, 0.0, 0.0]), np.array(box)), sq(0, 0))[0]) == 0


def test_zero_extent_boxes_in_general_position(oracle):
    """A zero-width and a zero-length box (box_scenes.ZERO_EXTENT) against each other and against ordinary boxes at
    continuous random poses: the oracle's SAT on its own corners equals the exact predicate for every pair, in both argument
    orders (the construction of test_gpu_boxes.py::test_zero_extent_pairs_on_the_device)."""
    rng = np.random.default_rng(7)
    boxes = [np.array(b) for b in B.ZERO_EXTENT + (B.CAR, B.SKEW[1])]
    hits = 0
    for n in range(4000):
        ba, bb = boxes[n % 2], boxes[rng.integers(4)]
        pa, pb = (np.array([*rng.uniform(-3, 3, 2), 0.0, rng.uniform(-3.2, 3.2), 0.0, 0.0]) for _ in range(2))
        A, Q = oracle.corners(pa, ba), oracle.corners(pb, bb)
        want = B.quads_meet_exact(A, Q)
        assert oracle.quads_intersect(A, Q) == want and oracle.quads_intersect(Q, A) == want, (n, pa, ba, pb, bb)
        hits += want
    assert 400 < hits < 3000


def test_scenes_hold_every_box_class_and_kind():
    """Every class of box_scenes (the giant included) occurs, with center_y of either sign; static entities, entities that
    appear late and entities that vanish early; the mixed scenes have pedestrian agents AND vehicles of every class."""
    for recipe in ("yard", "mixed"):
        scs = B.batch(recipe, 100)
        boxes = {tuple(b) for sc in scs for b in sc["bbox"]}
        assert set(B.SMALL) | {B.LORRY} <= boxes
        assert {np.sign(b[3]) for b in boxes} == {-1.0, 0.0, 1.0} and {np.sign(b[2]) for b in boxes} == {-1.0, 0.0, 1.0}
        n = np.concatenate([np.diff(sc["knot_off"]) for sc in scs])
        first = np.concatenate([sc["knots"][sc["knot_off"][:-1], 0] for sc in scs])
        last = np.concatenate([sc["knots"][sc["knot_off"][1:] - 1, 0] for sc in scs])
        assert (n == 1).sum() > 20 and ((n > 1) & (first > 0)).sum() > 20 and ((n > 1) & (last < scs[0]["length"])).sum() > 20
        if recipe == "mixed":
            ped = np.concatenate([sc["kind"] == B.KIND_AGENT_PEDESTRIAN for sc in scs])
            assert 0.3 < ped.mean() < 0.7
            assert set(B.SMALL[1:]) <= {tuple(b) for sc in scs for b, k in zip(sc["bbox"], sc["kind"]) if k != B.KIND_AGENT_PEDESTRIAN}
    assert {tuple(sc["bbox"][sc["giant"]]) for E in (3, 12, 48) for sc in B.batch("yard", E)} == set(B.GIANTS)
    far = B.batch("yard", 12, far=True)
    assert sorted({round(abs(sc["knots"][0, 1]) / 1e4) for sc in far}) == [3, 20, 75]


if __name__ == "__main__":  # the table above, from the generator: python tests/test_boxes_cpu.py
    from oracle import oracle as O

    O.build()
    for s in SCENES:
        t = _tally(O, s)
        assert not t[2]
        print(f'    "{scene_id(s)}": {(t[3] // 2).tolist()},  # near {t[0]}, meet {t[1]}, rational {t[6]}, cross {t[4]} / {t[5]}', flush=True)
