"""Scenes and parameter sets aimed at the GUARDS of the fast fp64 arithmetic of the pedestrian paths (RecipDiv in
csrc/sgym_core.hpp; FastArith, sg_exp, ped_pair in sgym_agents.hpp; crowd_pair, crowd_exp, sg_sqrt_core, crowd_sane,
crowd_params_ok in sgym_crowd.hpp) and of the PID derivative (pid_step), and a CPU restatement of those guards.
tests/test_arith_guards_cpu.py and tests/test_gpu_arith_guards.py use it.  A plain module, like box_scenes.py: numpy only,
deterministic; what needs the oracle (its exp, sincos and radius rule) takes the oracle module as an argument.

pair_terms() is ped_pair with ExactArith for ONE (pedestrian, neighbour) pair in the reference's operation order, in Python
floats (IEEE + - * /, math.sqrt, a once-rounded fma by exact rational arithmetic), and returns every intermediate a guard
looks at.  guard_class() names the guards that pair trips; every constant of the table below stands here once.

    near        hi word of min(a_rn, a_qn, a_b) < 2^-100          (crowd_pair: `bad`)
    faint       hi word of a_rep < 2^-700, rep == 0 included       (crowd_pair: `bad`)
    sliver      neither a >= cm + slack nor a <= cm - slack         (quotient_ge / crowd_pair: `bad`)
    negzero     a -0.0 numerator of a RecipDiv::div                 (RecipDiv::safe)
    numer       a non-zero numerator, biased exponent not in [64, 1983]
    denom       a divisor outside (2^-500, 2^500)                   (RecipDiv::ok)
    sqrt_range  a sqrt argument outside [2^-700, 2^1000)            (FastArith::sqrt)
    insane      per pedestrian and step: crowd_sane fails           (voted per tile)
    params      per parameter set: crowd_params_ok is false         (per launch)

Every scenario holds its aimed pedestrians at exactly representable coordinates near the origin and fills its other slots with
bystanders that stand more than a neighbour radius apart on a far row: they walk, they are nobody's neighbour.
"""
import math
import struct
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

KIND_AGENT_PID, KIND_AGENT_PEDESTRIAN = 3, 5
C_PED_SPEED_DESIRED, C_PED_HEAD_ROT, C_PED_RADIUS = 9, 11, 12
DT = 1.0 / 30.0
RADIUS = 3.0
SLOTS = 64  # entity slots of a batch: the all-pedestrian kernel runs tiles of 64 lanes, so the 2 .. 16 pedestrians of a scenario
            # are followed by padding slots (SG_KIND_NONE), which both the device and the oracle skip
PED_BOX = (0.69, 0.7, 0.0, 0.0)
CAR_BOX = (2.0, 4.2, 1.37, 0.0)
DEFAULT_CTRL = np.array([0.7, 5.0, np.nan, 0.0, 0.03054, 1.5709, 0.3753, 1.8970, 0.0204, 0.0, 5.0, 0.0, 1.0, 0, 0, 0])  # oracle.DEFAULT_CTRL
# sf[] layout of the oracle (oracle.social_force_params) == the fields of sg_social_force, in order
SF_TAU, SF_V, SF_SIGMA, SF_C, SF_SW, SF_SW_USE, SF_COS, SF_MAXF = range(8)

# ---- the constants of the guards, each named once -------------------------------------------------------------------------
HI_NEAR = 0x39B00000          # hi word of 2^-100: the first three sqrt arguments
HI_FAINT = 0x14300000         # hi word of 2^-700: |rep|^2
SLACK = 2.0 ** -50            # the sliver of the sight-weight decision, relative to |cos_sight * m|
NUMER_EXP = (64, 1983)        # biased exponents of a safe non-zero numerator
DENOM = (2.0 ** -500, 2.0 ** 500)       # open interval of safe divisors
SQRT_RANGE = (2.0 ** -700, 2.0 ** 1000)  # [lo, hi) in which the bare rsq + Goldschmidt core is the compiler's sqrt
SANE_LO, SANE_HI_COORD, SANE_HI_STEP = 2.0 ** -800, 2.0 ** 400, 2.0 ** 20
PARAM_RANGE = (2.0 ** -100, 2.0 ** 100)
EXP_CUTOFF = -745.13321910194110842
NEG_ZERO_BITS = 1 << 63


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def hi_word(x):
    """__double2hiint: the upper 32 bits as a signed int."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0] >> 32


def is_neg_zero(x):
    return bits(x) == NEG_ZERO_BITS


def nxt(x, n=1):
    """The n-th double above x (below for n < 0)."""
    x = float(x)
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def fma(a, b, c):
    """a * b + c rounded once: exact rational arithmetic and one correctly rounded conversion; IEEE signs of zero."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s != 0:
        r = float(s)
        return math.copysign(0.0, s) if r == 0.0 else r  # (an underflow keeps the sign)
    if p == 0 and c == 0.0:  # a signed zero product plus a signed zero: -0 only when both are
        return -0.0 if (math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0) else 0.0
    return 0.0  # exact cancellation, round to nearest: +0


def div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def sqrt(x):
    return math.sqrt(x) if x >= 0 else (x if x != x else math.nan)


def norm2(a, b):
    return sqrt(fma(b, b, a * a))


_LN2HI, _LN2LO, _INVLN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
_P = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06,
      4.13813679705723846039e-08)


def exp_parts(x):
    """sgo_exp / sg_exp restated: (value, numerator r * c, divisor 2 - c of its one quotient); the last two None where the
    function returns before it divides."""
    if x != x:
        return x, None, None
    if x > 709.782712893383973096:
        return math.inf, None, None
    if x < EXP_CUTOFF:
        return 0.0, None, None
    k = float(np.rint(x * _INVLN2))
    hi = x - k * _LN2HI
    lo = k * _LN2LO
    r = hi - lo
    t = r * r
    c = r - t * (_P[0] + t * (_P[1] + t * (_P[2] + t * (_P[3] + t * _P[4]))))
    y = 1.0 - ((lo - div(r * c, 2.0 - c)) - hi)
    return math.ldexp(y, int(k)), r * c, 2.0 - c


def pair_terms(O, px, py, ox, oy, ovx, ovy, dtn, sf, head_rot=0.0):
    """One neighbour's terms of SocialForce._step for the pedestrian at (px, py): ped_pair<false, false> with ExactArith, i.e.
    the oracle's loop body.  (ox, oy, ovx, ovy): the neighbour's position and velocity; dtn = next_t - t."""
    hs, hc = O.sincos(head_rot)
    T = {}
    vx, vy = fma(ovx, hc, ovy * (-hs)), fma(ovx, hs, ovy * hc)
    a_vn = fma(vy, vy, vx * vx)
    vn = sqrt(a_vn) + 0.0000000001
    ux, uy = div(vx, vn), div(vy, vn)
    rx, ry = px - ox, py - oy
    a_rn = fma(ry, ry, rx * rx)
    rn = sqrt(a_rn)
    vmag = norm2(ovx, ovy) + 0.0000000001
    odx, ody = div(ovx, vmag), div(ovy, vmag)
    step = vmag * dtn
    sx, sy = step * odx, step * ody
    qx, qy = rx - sx, ry - sy
    a_qn = fma(qy, qy, qx * qx)
    qn = sqrt(a_qn) + 0.0000000001
    sm = rn + qn
    a_b = sm * sm - step * step
    b = (1.0 / 2) * sqrt(a_b)
    k1 = (1.0 / 4) * div(1.0, b) * sm
    dbx, dby = k1 * (div(rx, rn) + div(qx, qn)), k1 * (div(ry, rn) + div(qy, qn))
    sigma = float(sf[SF_SIGMA])
    x_exp = div(-b, sigma)
    e_mine, rc, den = exp_parts(x_exp)
    k2 = div(float(sf[SF_V]), sigma) * O.exp(x_exp)
    repx, repy = k2 * dbx, k2 * dby
    k3 = 2 * float(sf[SF_C])
    attx, atty = k3 * rx, k3 * ry
    a_rep = fma(repy, repy, repx * repx)
    m = sqrt(a_rep) + 0.0000000001
    a = fma(uy, repy, ux * repx)
    cos_sight, sw = float(sf[SF_COS]), float(sf[SF_SW])
    a_att = fma(atty, atty, attx * attx)
    m2 = sqrt(a_att) + 0.0000000001
    a2 = fma(uy, atty, ux * attx)
    if sf[SF_SW_USE] != 0.0:
        w1 = 1.0 if div(a, m) >= cos_sight else sw
        w2 = 1.0 if div(a2, m2) >= cos_sight else sw
        c1, c2 = (w1 * repx, w1 * repy), (w2 * attx, w2 * atty)
    else:
        c1, c2 = (repx, repy), (attx, atty)
    rotated = not (hs == 0.0 and hc == 1.0)
    divs = [(1.0, b), (rx, rn), (ry, rn), (qx, qn), (qy, qn), (-b, sigma)]  # every (numerator, divisor) of the pair
    if rc is not None:
        divs.append((rc, den))
    if rotated:
        divs += [(vx, vn), (vy, vn)]
    T.update(a_vn=a_vn, vn=vn, v=(vx, vy), a_rn=a_rn, a_qn=a_qn, a_b=a_b, a_rep=a_rep, a=a, m=m, b=b, rn=rn, qn=qn)
    T.update(r=(rx, ry), q=(qx, qy), s=(sx, sy), step=step, x_exp=x_exp, exp_mine=e_mine, rc=rc, exp_den=den)
    T.update(rep=(repx, repy), c1=c1, c2=c2, divs=divs, a_att=a_att, m_att=m2, a2=a2, rotated=rotated)
    return T


def accumulate(fx, fy, T, sf):
    """ped_accumulate: the neighbour's terms join the force in the reference's order."""
    first, second = (T["c1"], T["c2"]) if sf[SF_SW_USE] != 0.0 else (T["c2"], T["c1"])
    fx += first[0]; fy += first[1]
    fx += second[0]; fy += second[1]
    return fx, fy


def goal_force(px, py, gx, gy, vdes, velx, vely, sf):
    """_force_to_goal, social_force.py:119-138."""
    ex, ey = gx - px, gy - py
    gn = norm2(ex, ey)
    if gn == 0:
        gn += 0.000000001
    inv_tau = div(1, float(sf[SF_TAU]))
    return inv_tau * (vdes * div(ex, gn) - velx), inv_tau * (vdes * div(ey, gn) - vely)


def _numerators(T, sf):
    out = [T["r"][0], T["r"][1], T["q"][0], T["q"][1], 1.0, -T["b"]]
    if T["rc"] is not None:
        out.append(T["rc"])
    if T["rotated"]:
        out += [T["v"][0], T["v"][1]]
    return out


def guard_class(T, sf):
    """The guards one active pair trips, from its pair_terms."""
    g = set()
    if min(hi_word(T["a_rn"]), hi_word(T["a_qn"]), hi_word(T["a_b"])) < HI_NEAR:
        g.add("near")
    if hi_word(T["a_rep"]) < HI_FAINT:
        g.add("faint")
    if sf[SF_SW_USE] != 0.0:
        cm = float(sf[SF_COS]) * T["m"]
        slack = abs(cm) * SLACK
        if not (T["a"] >= cm + slack) and not (T["a"] <= cm - slack):
            g.add("sliver")
    nums = _numerators(T, sf)
    if any(is_neg_zero(v) for v in nums):
        g.add("negzero")
    for v in nums:
        e = (bits(v) >> 52) & 0x7FF
        if v != 0.0 and not (NUMER_EXP[0] <= e <= NUMER_EXP[1]):
            g.add("numer")
    dens = [T["rn"], T["qn"], T["b"], float(sf[SF_SIGMA])] + ([T["exp_den"]] if T["exp_den"] is not None else [])
    if T["rotated"]:
        dens.append(T["vn"])
    if any(not (DENOM[0] < abs(d) < DENOM[1]) for d in dens):
        g.add("denom")
    args = [T["a_rn"], T["a_qn"], T["a_b"], T["a_rep"]] + ([T["a_vn"]] if T["rotated"] else [])
    if any(not (SQRT_RANGE[0] <= v < SQRT_RANGE[1]) for v in args):
        g.add("sqrt_range")
    return g


def sane(v, hi_bound):
    """crowd_sane: +0.0, or a magnitude in [2^-800, hi_bound).  (-0.0 is refused: px - ox is -0.0 only for px = -0.0, and a
    -0.0 numerator is what RecipDiv::div cannot take.)"""
    a = abs(v)
    return bits(v) == 0 or (a >= SANE_LO and a < hi_bound)


def insane(x, y, vx, vy, dtn):
    """The per-pedestrian, per-step guard of the crowd kernel (tile_collisions): coordinates and the products step * o."""
    vmag = norm2(vx, vy) + 0.0000000001
    stp = vmag * dtn
    sx, sy = stp * div(vx, vmag), stp * div(vy, vmag)
    return not (sane(x, SANE_HI_COORD) and sane(y, SANE_HI_COORD) and (sx == 0.0 or sane(abs(sx), SANE_HI_STEP))
                and (sy == 0.0 or sane(abs(sy), SANE_HI_STEP)) and stp < SANE_HI_STEP)


def params_bad(sf):
    """not crowd_params_ok."""
    sg, ac = float(sf[SF_SIGMA]), abs(float(sf[SF_COS]))
    k2s = abs(div(float(sf[SF_V]), sg))
    lo, hi = PARAM_RANGE
    return not (lo <= sg <= hi and (ac == 0.0 or lo <= ac <= hi) and k2s <= hi and sf[SF_C] == 0.0 and sf[SF_SW] > 0.0
                and sf[SF_SW_USE] != 0.0)


def default_sf(**kw):
    """SocialForceParameters defaults in the sf[] layout; cos_sight raw."""
    sf = np.array([1.5, 1.0, 1.0, 0.0, 0.5, 1.0, float(np.cos(200 / 2 * np.pi / 180)), 1.3, 0.0, 0.0, 2.0, 0.1], np.float64)
    for k, v in kw.items():
        sf[{"tau": SF_TAU, "V": SF_V, "sigma": SF_SIGMA, "C": SF_C, "sw": SF_SW, "sw_use": SF_SW_USE, "cos": SF_COS}[k]] = v
    return sf


# ---- scenes ---------------------------------------------------------------------------------------------------------------
@dataclass
class Scene:
    """One scenario.  peds [n, 5]: x, y, goal x, goal y, desired speed; vel [n, 2]: the velocity the knots give at the reset;
    pairs: the aimed (pedestrian, neighbour) pairs; expect: guards every aimed pair must trip at the first step; clean: the
    aimed pairs trip nothing there (the "just passes" twin); nan: the pedestrians whose rows may be NaN; past: the knots lie
    before the start and the scene runs with persist (the only way a -0.0 coordinate survives the interpolation)."""
    name: str
    peds: np.ndarray
    pairs: tuple = ((0, 1), (1, 0))
    expect: frozenset = frozenset()
    clean: bool = False
    nan: tuple = ()
    vel: np.ndarray = None
    past: bool = False
    want_insane: tuple = ()   # pedestrians that must fail the per-step guard at the first step
    want_sane: tuple = ()     # ... and those that must pass it


@dataclass
class Family:
    """Scenes that share entity slots, steps, head rotation; param_sets: the sf[] arrays the whole batch is run under, one
    after the other (one parameter set per handle: the crowd kernel holds one)."""
    name: str
    scenes: list
    E: int
    steps: int = 4
    param_sets: list = field(default_factory=lambda: [("default", default_sf())])
    head_rot: float = 0.0
    car: bool = False
    guard: str = ""           # the aimed guard (per pair, or "insane" / "params")
    rest_vel: tuple = None    # the velocity at the reset of every pedestrian whose scene gives none
    want_params_bad: dict = field(default_factory=dict)  # parameter-set name -> params_bad expected

    @property
    def past(self):
        return any(s.past for s in self.scenes)


def ped(x, y, gx=None, gy=None, vdes=1.3):
    return [x, y, x if gx is None else gx, y - 6.0 if gy is None else gy, vdes]


def bystanders(n, k0=0):
    """n pedestrians on a far row, 8 m apart (more than the neighbour radius), each walking its own way."""
    return [ped(24.0 + 8.0 * (k0 + k), 40.0, 24.0 + 8.0 * (k0 + k) + (k % 3 - 1) * 2.0, 34.0 + (k % 2) * 12.0, 0.9 + 0.1 * (k % 5))
            for k in range(n)]


def place(aimed, E, slots):
    """The aimed pedestrians in the given slots of an E-slot scenario, bystanders everywhere else."""
    rows = bystanders(E)
    for a, s in zip(aimed, slots):
        rows[s] = a
    return np.array(rows, np.float64)


def pack(fam, scenes=None):
    """The batch of a family in the sg_scenarios layout (the fields of PackedScenarios, as a dict)."""
    scenes = fam.scenes if scenes is None else scenes
    R, E0 = len(scenes), fam.E
    c = 1 if fam.car else 0
    E = max(E0 + c, SLOTS)  # padding slots (SG_KIND_NONE) behind the pedestrians
    T = (fam.steps + 2) * DT  # (the rollout ends by its step count, not by the scenario's length)
    kind = np.full((R, E), KIND_AGENT_PEDESTRIAN, np.int32)
    etype = np.ones((R, E), np.int32)
    bbox = np.tile(np.array(PED_BOX), (R, E, 1))
    ctrl = np.tile(DEFAULT_CTRL, (R, E, 1))
    knots = np.zeros((R, E, 2, 7))
    routes, route_n = [], np.full((R, E), 2, np.int64)
    kind[:, c + E0:], etype[:, c + E0:], route_n[:, c + E0:] = 0, 0, 0
    for r, s in enumerate(scenes):
        assert s.peds.shape == (E0, 5), (fam.name, s.name, s.peds.shape)
        t0, t1 = (-2.0, -1.0) if s.past else (0.0, T)
        knots[r, :, 0, 0], knots[r, :, 1, 0] = t0, t1
        knots[r, c:c + E0, :, 1:3] = s.peds[:, None, 0:2]
        vel = s.vel if s.vel is not None else fam.rest_vel
        if vel is not None and not s.past:  # (knots before the start: the velocity at the reset is zero)
            knots[r, c:c + E0, 1, 1:3] += np.asarray(vel) * T
        ctrl[r, c:c + E0, C_PED_SPEED_DESIRED] = s.peds[:, 4]
        ctrl[r, c:c + E0, C_PED_RADIUS] = RADIUS
        ctrl[r, c:c + E0, C_PED_HEAD_ROT] = fam.head_rot
        if fam.car:  # synthetic.make_crowd_with_car's recipe: slot 0 is a PID car on a straight line, far from the crowd
            kind[r, 0], etype[r, 0], bbox[r, 0], route_n[r, 0] = KIND_AGENT_PID, 0, CAR_BOX, 0
            knots[r, 0, 0] = [0.0, -30.0, 500.0, 0.0, 0.0, 0.0, 0.0]
            knots[r, 0, 1] = [T, -30.0 + 5.0 * T, 500.0, 0.0, 0.0, 0.0, 0.0]
        routes.append(np.stack([s.peds[:, 0:2], s.peds[:, 2:4]], axis=1).reshape(-1, 2))
    return dict(
        n_scenarios=R, n_entities=E, kind=kind.ravel(), etype=etype.ravel(), bbox=bbox.reshape(-1, 4),
        knot_off=np.arange(R * E + 1, dtype=np.int64) * 2, knots=knots.reshape(-1, 7), ego=np.zeros(R, np.int32),
        t0=np.zeros(R), length=np.full(R, T), ctrl=ctrl.reshape(-1, 16),
        route_off=np.concatenate([[0], np.cumsum(route_n.ravel())]).astype(np.int64), routes=np.concatenate(routes))


def run_oracle(O, fam, batch, r, sf, noise=None):
    """Scenario r of a packed family through the oracle, every step recorded."""
    E = batch["n_entities"]
    sl = slice(r * E, (r + 1) * E)
    ko, ro = batch["knot_off"], batch["route_off"]
    return O.rollout(ko[r * E:(r + 1) * E + 1] - ko[r * E], batch["knots"][ko[r * E]:ko[(r + 1) * E]], batch["bbox"][sl],
                     batch["etype"][sl], batch["kind"][sl], 0, 0.0, float(batch["length"][r]), DT, persist=fam.past,
                     ctrl=batch["ctrl"][sl], max_steps=fam.steps, route_off=ro[r * E:(r + 1) * E + 1] - ro[r * E],
                     routes=batch["routes"][ro[r * E]:ro[(r + 1) * E]], sf=sf, event_cap=256, noise=noise)


def active_pairs(O, fam, o, k):
    """The (pedestrian, neighbour) pairs the oracle evaluates in the step from record row k: indices of the scene's pedestrians
    (a car in slot 0 does not count), in the oracle's order."""
    c = 1 if fam.car else 0
    P = o["poses"][k][:fam.E + c]
    out = []
    with np.errstate(all="ignore"):
        close = np.hypot(P[:, None, 0] - P[None, :, 0], P[:, None, 1] - P[None, :, 1]) < RADIUS * 1.01  # (prefilter only)
    for i, j in zip(*np.nonzero(close)):
        if i >= c and j >= c and j != i and O.in_radius(P[i, 0], P[i, 1], RADIUS, P[j, 0], P[j, 1]):
            out.append((int(i) - c, int(j) - c))
    return out


def terms_of(O, fam, o, k, i, j, sf):
    c = 1 if fam.car else 0
    P, V = o["poses"][k], o["vels"][k]
    dtn = float(o["t"][k + 1] - o["t"][k])
    return pair_terms(O, P[i + c, 0], P[i + c, 1], P[j + c, 0], P[j + c, 1], V[j + c, 0], V[j + c, 1], dtn, sf, fam.head_rot)


# ---- the families ---------------------------------------------------------------------------------------------------------
P50 = 2.0 ** -50
SUBNORMAL = 3 * 5e-324
NEAR_SEPS = (("coincident", 0.0), ("2^-50", P50), ("below 2^-50", nxt(P50, -1)), ("2^-60", 2.0 ** -60), ("2^-300", 2.0 ** -300),
             ("subnormal", SUBNORMAL),
             # squares of about 2^-1009 and 2^-1029 (subnormal): the residuals of the bare sqrt core underflow there
             ("1.37 * 2^-505", 1.37 * 2.0 ** -505), ("1.37 * 2^-515", 1.37 * 2.0 ** -515))


def near_scenes(E):
    out = []
    for dname, (dx, dy) in (("x", (1.0, 0.0)), ("y", (0.0, 1.0)), ("diag", (1.0, 1.0))):
        for sname, s in NEAR_SEPS:
            for slots in ((0, 1), (0, E - 1)):
                A, B = ped(0.0, 0.0, 4.0, 5.0), ped(s * dx, s * dy, -5.0, 4.0, 1.1)
                on_axis = dname != "diag"
                coincident = s == 0.0 or s == SUBNORMAL  # (a subnormal separation squares to 0: the same zero norm, 0 / 0)
                passes = s == P50 or (dname == "diag" and s == nxt(P50, -1))  # (diagonal: a_rn = 2 s^2 >= 2^-100 from s = 2^-50.5)
                out.append(Scene(f"near {dname} {sname} slots {slots}", place([A, B], E, slots), pairs=(slots, slots[::-1]),
                                 expect=frozenset() if passes else frozenset({"near"}), clean=passes and on_axis,
                                 nan=slots if coincident else ()))
    return out


def negzero_scenes(E, lattice=True):
    """Pedestrians on the lines x = +-0.0 and y = +-0.0 with goals on the same line, every sign combination of (owner,
    neighbour); desired speeds of either sign and -0.0 (a goal force component is -0.0 only for a negative or -0.0 desired speed
    or a -0.0 goal coordinate: then the sign of a zero repulsion component decides the sign of the force component, and the
    heading atan2(+-0, negative) is +-pi); one pair walks in the -x direction with a zero y chain."""
    out = []
    Z = (0.0, -0.0)
    for axis in ("x", "y"):
        for za in Z:
            for zb in Z:
                for vdes in (1.3, -0.0, -1.3):
                    if axis == "x":  # on the line x = 0, walking along y
                        A, B = ped(za, 1.0, za, -5.0, vdes), ped(zb, -1.0, zb, 5.0, vdes)
                    else:            # on the line y = 0, A left of B; goals further along -x: a walk in the -x direction
                        A, B = ped(-1.0, za, -7.0, za, vdes), ped(1.0, zb, -6.0, zb, vdes)
                    # px - ox is -0.0 only for px = -0.0 and ox = +0.0: the one direction of the pair that trips the guard
                    tripped = is_neg_zero(za) != is_neg_zero(zb)
                    for slots in ((0, 1), (0, E - 1)):
                        pairs = (slots, slots[::-1]) if not tripped else ((slots,) if is_neg_zero(za) else (slots[::-1],))
                        out.append(Scene(f"negzero line {axis}=0 owner {za!r} neighbour {zb!r} vdes {vdes!r} slots {slots}",
                                         place([A, B], E, slots), pairs=pairs,
                                         expect=frozenset({"negzero"}) if tripped else frozenset(), past=True))
    if lattice and E >= 9:  # 3 x 3 around the origin, -0.0 centre coordinates, goals on the own row / column
        for vdes in (1.3, -0.0):
            rows = []
            for iy in (-1, 0, 1):
                for ix in (-1, 0, 1):
                    x, y = (ix * 1.0 if ix else -0.0), (iy * 1.0 if iy else -0.0)
                    rows.append(ped(x, y, x - 6.0 if iy == 0 else x, y if iy == 0 else y - 6.0 * iy, vdes))
            out.append(Scene(f"negzero lattice vdes {vdes!r}", place(rows, E, range(9)), pairs=((1, 4), (3, 4), (5, 4), (7, 4)),
                             expect=frozenset(), past=True))
    return out


def midpoint_scenes(E):
    """Rounding-hard operands: separations x = 2^k - j ulp (rn = x: an all-ones mantissa divisor for j = 1, and sqrt arguments
    fl(x^2) next to the squares of neighbouring doubles), on either axis."""
    out = []
    for k in (1, 0, -2):
        for j in range(1, 9):
            x = nxt(2.0 ** k, -j)
            for axis in ("x", "y"):
                B = ped(x, 0.0, -5.0, 4.0, 1.1) if axis == "x" else ped(0.0, x, -5.0, 4.0, 1.1)
                out.append(Scene(f"midpoint 2^{k} - {j} ulp along {axis}", place([ped(0.0, 0.0, 4.0, 5.0), B], E, (0, 1))))
    return out


ONES = nxt(1.0, -1)  # 1 - 2^-53: x / ONES lies next to a rounding midpoint for small-mantissa x
CLUSTER = [ped(0.0, 0.0, 4.0, 5.0), ped(1.5, 0.0, -5.0, 4.0, 1.1), ped(0.25, 1.75, 0.25, -6.0, 1.2), ped(-1.0, -0.75, 6.0, 1.0, 1.0)]
CLUSTER_PAIRS = tuple((i, j) for i in range(4) for j in range(4) if i != j)
CLUSTER_VEL = np.array([[0.5, 0.25], [-0.75, 0.5], [0.125, -1.0], [1.0, 0.375]])


def cluster_scene(E, name, **kw):
    vel = np.zeros((E, 2))
    vel[:4] = CLUSTER_VEL
    return Scene(name, place(CLUSTER, E, range(4)), pairs=CLUSTER_PAIRS, vel=vel, **kw)


def solve_sigma(O, T_of, lo, hi, pred):
    """Adjacent doubles (s0, s1 = next above s0) in [lo, hi] with pred(T_of(s0)) != pred(T_of(s1)), by bisection on the bit
    pattern (pred differs at the ends)."""
    a, b = bits(lo), bits(hi)
    pa = pred(T_of(lo))
    assert pa != pred(T_of(hi))
    while b - a > 1:
        mid = (a + b) // 2
        s = struct.unpack("<d", struct.pack("<Q", mid))[0]
        if pred(T_of(s)) == pa:
            a = mid
        else:
            b = mid
    f = lambda u: struct.unpack("<d", struct.pack("<Q", u))[0]  # noqa: E731
    return f(a), f(b)


def faint_params(O):
    """ped_repulse_sigma such that, for the pair (0, 0) - (2, 0) at rest, |rep|^2 crosses 2^-700 and -b / sigma crosses the
    exp cutoff: the double on either side of each crossing, and one further out."""
    def T_of(s):
        return pair_terms(O, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, DT, default_sf(sigma=s))

    f0, f1 = solve_sigma(O, T_of, 2.0 / 300.0, 2.0 / 200.0, lambda T: hi_word(T["a_rep"]) < HI_FAINT)
    c0, c1 = solve_sigma(O, T_of, 2.0 / 800.0, 2.0 / 700.0, lambda T: T["x_exp"] < EXP_CUTOFF)
    return [(f"sigma {n}", default_sf(sigma=s)) for n, s in
            (("faint-", nxt(f0, -1)), ("faint0", f0), ("faint1", f1), ("faint+", nxt(f1, 1)),
             ("cutoff-", nxt(c0, -1)), ("cutoff0", c0), ("cutoff1", c1), ("cutoff+", nxt(c1, 1)))]


def faint_scenes(E):
    return [Scene(f"faint slots {slots}", place([ped(0.0, 0.0, 4.0, 5.0), ped(2.0, 0.0, -5.0, 4.0, 1.1)], E, slots),
                  pairs=(slots, slots[::-1])) for slots in ((0, 1), (0, E - 1))]


# (neighbour x, y, its velocity x, y) of two-pedestrian scenes, owner at the origin, found by a search over 480 such scenes on
# sixteenths of a metre and eighths of a m/s: with cos_sight = q = fl(a / m), fl(q * m) > a, so that a compare WITHOUT the slack
# (a >= cos_sight * m) says "no" where IEEE's fl(a / m) >= cos_sight says "yes".  13 of the 480 had the property.
SLIVER_HARD = ((1.625, -0.875, -0.125, 0.875), (-1.1875, -1.875, 1.25, 0.0), (0.875, 1.3125, 1.0, -0.5), (1.4375, -1.0, -0.25, 1.5),
               (0.75, -0.6875, -1.125, -1.25), (-1.75, -1.9375, 1.25, -0.125))


def sliver_scenes(E):
    out = [cluster_scene(E, "cluster")]
    for bx, by, vx, vy in SLIVER_HARD:
        vel = np.zeros((E, 2))
        vel[:2] = [[0.5, 0.25], [vx, vy]]
        out.append(Scene(f"sliver hard pair {(bx, by, vx, vy)}", place([ped(0.0, 0.0, 4.0, 5.0), ped(bx, by, -5.0, 4.0, 1.1)], E, (0, 1)),
                         pairs=((0, 1),), vel=vel))
    return out


def sliver_params(O, fam):
    """cos_sight on and beside fl(a / m) of the aimed pair (owner 0, neighbour 1 of the cluster, from the state at the reset:
    a and m do not depend on cos_sight), and the special values."""
    batch = pack(fam)
    o = run_oracle(O, fam, batch, 0, default_sf())
    T = terms_of(O, fam, o, 0, 0, 1, default_sf())
    q = div(T["a"], T["m"])
    assert q == q and 0.0 < abs(q) < 1.0, q
    vals = [("q", q), ("q-1ulp", nxt(q, -1)), ("q+1ulp", nxt(q, 1))]
    for n, f in (("q(1+2^-50)", 1.0 + SLACK), ("q(1-2^-50)", 1.0 - SLACK)):
        v = q * f
        vals += [(n, v), (n + "-1ulp", nxt(v, -1)), (n + "+1ulp", nxt(v, 1))]
    for i, j in fam.scenes[0].pairs:  # the threshold of every other pair of the cluster
        if (i, j) != (0, 1):
            Tij = terms_of(O, fam, o, 0, i, j, default_sf())
            vals.append((f"q of pair {i}-{j}", div(Tij["a"], Tij["m"])))
    for r in range(1, len(fam.scenes)):  # the hard pairs: their own thresholds
        Tr = terms_of(O, fam, run_oracle(O, fam, batch, r, default_sf()), 0, 0, 1, default_sf())
        vals.append((f"q of hard pair {r}", div(Tr["a"], Tr["m"])))
    vals += [("0", 0.0), ("-0", -0.0), ("2^-100", 2.0 ** -100), ("-2^-100", -(2.0 ** -100)), ("1", 1.0), ("-1", -1.0)]
    return [(f"cos_sight {n}", default_sf(cos=v)) for n, v in vals], q


def params_sets():
    """(name, sf, crowd_params_ok must fail)"""
    P = []
    lo, hi = PARAM_RANGE
    for n, s, bad in (("sigma 2^-100", lo, False), ("sigma below 2^-100", nxt(lo, -1), True), ("sigma 2^100", hi, False),
                      ("sigma above 2^100", nxt(hi, 1), True)):
        P.append((n, default_sf(sigma=s), bad))
    P.append(("V/sigma 2^100", default_sf(V=hi), False))
    P.append(("V/sigma above 2^100", default_sf(V=nxt(hi, 1)), True))
    for c in (0.0, -0.0, 5e-324):
        P.append((f"attract_C {c!r}", default_sf(C=c), c != 0.0))
    for w in (5e-324, 0.0, -0.5):
        P.append((f"sight_weight {w!r}", default_sf(sw=w), not w > 0.0))
    P.append(("sight weights off", default_sf(sw_use=0.0), True))
    return P


def midpoint_sigma_sets():
    return [(f"sigma (1 - 2^-53) * 2^{k}", default_sf(sigma=ONES * 2.0 ** k)) for k in (0, -3, 2)]


INSANE_COORDS = (("2^-800", SANE_LO, False), ("below 2^-800", nxt(SANE_LO, -1), True), ("5e-324", 5e-324, True),
                 ("2^399", 2.0 ** 399, False), ("below 2^400", nxt(SANE_HI_COORD, -1), False), ("2^400", SANE_HI_COORD, True),
                 ("nan", math.nan, True))


def insane_scenes(E, slot=2):
    """A present pedestrian (slot `slot`) with one coordinate on either side of crowd_sane's bounds beside the cluster pairs,
    and one whose step product exceeds 2^20 (its knots give it a speed no controller would)."""
    out = []
    for n, v, bad in INSANE_COORDS:
        for axis in ("x", "y"):
            C = ped(v, 0.5, v, -6.0) if axis == "x" else ped(0.5, v, 6.0, v)
            rows = [ped(0.0, 0.0, 4.0, 5.0), ped(1.5, 0.0, -5.0, 4.0, 1.1)]
            s = Scene(f"insane {axis} = {n} in slot {slot}", place(rows + [C], E, (0, 1, slot)), pairs=((0, 1), (1, 0)),
                      nan=(slot,) if v != v else (), want_insane=(slot,) if bad else (), want_sane=() if bad else (slot,))
            out.append(s)
    vel = np.zeros((E, 2))
    vel[slot] = [4.0e7, 0.0]
    out.append(Scene(f"insane step product in slot {slot}", place([ped(0.0, 0.0, 4.0, 5.0), ped(1.5, 0.0, -5.0, 4.0, 1.1),
                                                                    ped(0.5, 1.0, 0.5, -6.0)], E, (0, 1, slot)),
                     pairs=((0, 1), (1, 0)), vel=vel, want_insane=(slot,)))
    return out


def families(O):
    """Every family of the suite, by name.  (O: the oracle module; the faint and sliver parameter sets are solved from
    pair_terms.)"""
    F = {}
    F["near"] = Family("near", near_scenes(4), 4, guard="near")
    F["negzero"] = Family("negzero", negzero_scenes(12), 12, steps=8, guard="negzero")
    F["midpoint"] = Family("midpoint", midpoint_scenes(3), 3, guard="")
    F["midpoint_sigma"] = Family("midpoint_sigma", [cluster_scene(6, "cluster")] + midpoint_scenes(6)[::8], 6,
                                 param_sets=midpoint_sigma_sets())
    F["faint"] = Family("faint", faint_scenes(5), 5, steps=3, param_sets=faint_params(O), guard="faint")
    sl = Family("sliver", sliver_scenes(6), 6, steps=3, guard="sliver")
    sl.param_sets, sl.q = sliver_params(O, sl)
    F["sliver"] = sl
    F["insane"] = Family("insane", insane_scenes(6), 6, steps=3, guard="insane")
    ps = params_sets()
    F["params"] = Family("params", [cluster_scene(5, "cluster")] + faint_scenes(5)[:1], 5, steps=3,
                         param_sets=[(n, sf) for n, sf, _ in ps], guard="params", want_params_bad={n: b for n, _, b in ps})
    # head rotation != 0: ped_pair<false, false> with FastArith::div2 on the rotated velocity; and with a car in slot 0, which
    # takes the scenario out of the all-pedestrian kernel
    for car in (False, True):
        tag = "headrot_car" if car else "headrot"
        F[tag + "_near"] = Family(tag + "_near", near_scenes(4)[::2], 4, head_rot=0.3, car=car, guard="near", rest_vel=(0.5, -0.25))
        F[tag + "_negzero"] = Family(tag + "_negzero", negzero_scenes(4, lattice=False)[::2], 4, steps=8, head_rot=0.3, car=car,
                                     guard="negzero")
        F[tag + "_midpoint"] = Family(tag + "_midpoint", midpoint_scenes(3)[::3], 3, head_rot=-0.7, car=car, rest_vel=(-0.375, 0.75))
    # two wavefronts per scenario, the aimed pair split across them; and the wide path (ExactArith throughout)
    for E, every in ((70, 1), (520, 3)):
        F[f"wide{E}"] = Family(f"wide{E}", (near_scenes(E)[1::2] + negzero_scenes(E, lattice=False)[1::2])[::every]
                               + insane_scenes(E, slot=E - 2)[10:], E, steps=3)
    return F


# ---- the PID derivative -----------------------------------------------------------------------------------------------------
# pid_step divides both error differences by State.dt through RecipDiv(State.dt) when both are `safe` numerators and State.dt
# a safe divisor, else by IEEE '/'.  One PID ego (slot 0) and two parked cars.  The divisor is State.dt = t - prev_t, NOT the
# timestep: 0.1 in the first step (State.reset sets prev_t = t - 0.1), then the difference of two accumulated clocks, which
# keeps the timestep's mantissa only while k * timestep is exact.  PID_DT_48 (1/30 rounded to 48 bits) keeps it for all 12
# steps; nextafter(1/32, 0) keeps its all-ones mantissa in steps 1 and 2 and decays to 2^-5 afterwards.
KIND_REPLAY = 1
PID_E, PID_STEPS = 3, 12
PID_DT_ONES = nxt(1.0 / 32.0, -1)   # an all-ones mantissa divisor (steps 1 and 2)
PID_DT_48 = float(round((1.0 / 30.0) * 2.0 ** 52)) * 2.0 ** -52  # mantissa of 48 bits: k * dt is exact for k <= 16
# the ego's controller row of the "d:" scenes: the derivative terms ARE the output (no P, no I term, limits out of reach)
PID_D_GAINS = {0: 0.7, 1: 50.0, 4: 0.0, 5: 0.4, 6: 0.0, 7: 1.0, 8: 0.0}
PID_DT_TINY, PID_DT_HUGE = 2.0 ** -600, 2.0 ** 600  # outside RecipDiv's divisor range (2^-500, 2^500): the IEEE branch
PID_T1 = 2.0 ** -7                  # end of the "lateral -0.0" ego's trajectory, before the first step ends


def pid_scene(name, dt):
    """knots [n, 7] per entity and the persist flag.  "moving": the ego's path bends, so both errors and both differences are
    ordinary numbers; "rest": it stands on its target, the differences are +0.0; "lat-0": persist, the path ends before the first
    step does, at y = -0.0 from y = +0.0 at heading 0: the first lateral error is -0.0 and so is its difference; "d:<slope>":
    the path leaves the heading from the start and the ego has PID_D_GAINS."""
    T = (PID_STEPS + 2) * dt
    if name.startswith("d:"):  # one straight segment that leaves the ego's heading from t = 0: both errors change in every step
        ego = [[0.0, 0.0, 0.0, 0, 0, 0, 0], [T, 5.0 * T, float(name[2:]) * T, 0, 0, 0, 0]]
    elif name.startswith("moving"):  # "moving:<slope>": how far the second half of the path leaves the first one's line
        bend = float(name.split(":")[1]) if ":" in name else 0.5
        ego = [[0.0, 0.0, 0.0, 0, 0, 0, 0], [T / 4, 1.25 * T, 0.0, 0, 0, 0, 0], [T, 5.0 * T, bend * T, 0, 0, 0, 0]]
    elif name == "rest":
        ego = [[0.0, 3.0, -2.0, 0, 0.25, 0, 0], [T, 3.0, -2.0, 0, 0.25, 0, 0]]
    else:
        ego = [[0.0, 0.0, 0.0, 0, 0, 0, 0], [PID_T1, 1.0, -0.0, 0, 0, 0, 0]]
    cars = [[[0.0, 100.0, 100.0 + 10.0 * k, 0, 0, 0, 0], [T, 100.0, 100.0 + 10.0 * k, 0, 0, 0, 0]] for k in range(PID_E - 1)]
    return [np.array(ego, np.float64)] + [np.array(c, np.float64) for c in cars], name == "lat-0"


def pid_groups(huge_moving):
    """(timestep, scene names): what runs under which timestep.  huge_moving: the largest timestep the moving ego stays finite
    under in the oracle (test_arith_guards_cpu.py finds and pins it); the ego at rest takes 2^600."""
    bends = tuple(f"moving:{b}" for b in (0.125, 0.3, -0.7, 1.1, -0.05, 0.9))
    return [(PID_DT_ONES, ("moving", "rest") + bends + PID_D_SCENES), (PID_DT_48, ("moving",) + PID_D_SCENES), (PID_DT_ONES, ("lat-0",)), (PID_DT_TINY, ("moving", "rest")), (PID_DT_HUGE, ("rest",)),
            (huge_moving, ("moving",))]


PID_D_SCENES = tuple(f"d:{b}" for b in (0.37, -0.81, 1.3, 0.055, -2.1, 0.64, -0.29, 1.9))
PID_HUGE_MOVING = 2.0 ** 254  # pinned by test_arith_guards_cpu.py: under 2^255 the squared length of a step overflows


def pid_pack(dt, names):
    scenes = [pid_scene(n, dt) for n in names]
    persist = any(p for _, p in scenes)
    R, E = len(scenes), PID_E
    kn = [k for sc, _ in scenes for k in sc]
    kind = np.full((R, E), KIND_REPLAY, np.int32)
    kind[:, 0] = KIND_AGENT_PID
    T = (PID_STEPS + 2) * dt
    ctrl = np.tile(DEFAULT_CTRL, (R, E, 1))
    for r, n in enumerate(names):
        if n.startswith("d:"):
            for col, v in PID_D_GAINS.items():
                ctrl[r, 0, col] = v
    return dict(n_scenarios=R, n_entities=E, kind=kind.ravel(), etype=np.zeros(R * E, np.int32), bbox=np.tile(np.array(CAR_BOX), (R * E, 1)),
                knot_off=np.concatenate([[0], np.cumsum([len(k) for k in kn])]).astype(np.int64), knots=np.concatenate(kn),
                ego=np.zeros(R, np.int32), t0=np.zeros(R), length=np.full(R, T), ctrl=ctrl.reshape(-1, 16)), persist


def pid_oracle(O, batch, persist, r, dt):
    E = batch["n_entities"]
    sl = slice(r * E, (r + 1) * E)
    ko = batch["knot_off"]
    return O.rollout(ko[r * E:(r + 1) * E + 1] - ko[r * E], batch["knots"][ko[r * E]:ko[(r + 1) * E]], batch["bbox"][sl], batch["etype"][sl],
                     batch["kind"][sl], 0, 0.0, float(batch["length"][r]), dt, persist=persist, ctrl=batch["ctrl"][sl], max_steps=PID_STEPS,
                     event_cap=256)


# ---- sg_log's small-|f| branch ------------------------------------------------------------------------------------------------
# The Box-Muller transform of the device noise takes log(u1) of a 53-bit uniform; fdlibm's log has a branch of its own for
# |f| < 2^-20 (the normalised argument within 2^-20 of 1), which a uniform enters about once in 700,000 draws.  Found by a
# search over seeds 1 .. 200,000 x entities 0 .. 5 x steps 0 .. 2 of scenario 0 (10 hits): (seed, entity, step, u1).  The first
# has k == 0 after the normalisation (log = f - R), the second k == -1 (dk * ln2_hi - ((R - dk * ln2_lo) - f)).
LOG_SMALL_F = ((1379, 5, 0, 0.9999991015336771), (22376, 2, 2, 0.5000002241523815))
LOG_STD = (0.1, 0.05)  # std_lon, std_lat of the noise scene


def philox_uniforms(seed, scenario, entity, step):
    """The two uniforms behind sg_noise_pair / sgo_noise_pair: Philox4x32-10 at counter (entity, step, 0, 0) under key
    (seed_lo ^ scenario, seed_hi), 53 bits each, in (0, 1)."""
    M = 0xFFFFFFFF
    c0, c1, c2, c3 = entity & M, step & M, 0, 0
    k0, k1 = (seed & M) ^ scenario, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return (float(((c0 << 32) | c1) >> 11) + 0.5) * 2.0 ** -53, (float(((c2 << 32) | c3) >> 11) + 0.5) * 2.0 ** -53


def log_takes_small_f_branch(x):
    """The test at the head of sgo_log / sg_log: (0x000fffff & (2 + hx)) < 3 on the mantissa's upper 20 bits."""
    hx = (bits(x) >> 32) & 0x000FFFFF
    return (0x000FFFFF & (2 + hx)) < 3


def log_family():
    return Family("log_small_f", [cluster_scene(6, "cluster")], 6, steps=3)
