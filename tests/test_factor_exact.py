"""The visual, LiDAR and prior factors and the two Plus operations against exact references (tests/factor_exact.py: mpmath at 50 digits, written from the
reference's text) on the named cases of tests/factor_cases.py. The references take a few seconds for the whole list and are computed here once.

Error measure, as for the IMU chain: per output group (the residual, then each Jacobian block as a whole) max|got - exact| / scale, scale = the larger of
max|exact| and the group's largest term as factor_exact returns it. CPU tests pin the oracle with bounds from rounding analysis (stated at each bound) and
yield the oracle's error per case and group; GPU tests allow the device four times that error plus 16 eps of the same scale, through the Ceres-layout hooks.
The identities that hold to the bit are asserted as such. Measured figures: DESIGN.md 6f."""
import copy
import ctypes as C
import functools
import numpy as np
import pytest
import factor_cases as fc
import factor_exact as fx
from vil_fusion_amd import abi, synth

EPS = float(np.finfo(np.float64).eps)
FACTOR = 4.0
FLOOR = 16.0 * EPS
# every output is a sum of a few products whose factors are themselves short sums (at most about 60 rounded operations deep, the extrinsic block of the
# projection factor); each operation errs by at most eps / 2 of a magnitude the scale dominates: 64 eps of the scale
CPU_BOUND = 64.0 * EPS


# ---- shared data (computed once, never modified) --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sets():
    import oracle_lib
    return fc.option_sets(oracle_lib.default_options())


@functools.lru_cache(maxsize=None)
def cases(family):
    return {"projection": lambda: fc.projection_cases(sets()), "projection_td": lambda: fc.projection_td_cases(sets()), "lidar": lambda: fc.lidar_cases(sets()),
            "edge": fc.edge_cases, "surf": fc.surf_cases, "pose_plus": fc.pose_plus_cases, "se3_plus": fc.se3_plus_cases, "prior": fc.prior_cases}[family]()


def _pack(groups, terms):
    """group -> (hi, lo, scale)"""
    out = {}
    for g, xs in groups.items():
        hi, lo = fx.to_dd(xs)
        out[g] = (hi, lo, max(float(np.abs(hi).max(initial=0.0)), terms[g]))
    return out


@functools.lru_cache(maxsize=None)
def exact(family, name):
    c = cases(family)[name]
    if family == "projection":
        o = sets()[c["opt"]]
        return _pack(*fx.projection_exact(o.focal_length, c["params"], c["pts_i"], c["pts_j"]))
    if family == "projection_td":
        o = sets()[c["opt"]]
        return _pack(*fx.projection_td_exact(o.focal_length, o.TR, o.ROW, c["params"], c["pts_i"], c["pts_j"], c["vel_i"], c["vel_j"], c["td_i"], c["td_j"],
                                             c["row_i"], c["row_j"]))
    if family == "lidar":
        o = sets()[c["opt"]]
        return _pack(*fx.lidar_between_exact(o.RIC[:], o.TIC[:], o.RCL[:], o.TCL[:], c["params"], c["q"], c["t"]))
    if family == "edge":
        return _pack(*fx.edge_exact(c["pose"], c["cp"], c["a"], c["b"]))
    if family == "surf":
        return _pack(*fx.surf_exact(c["pose"], c["cp"], c["n"], c["d"]))
    if family == "pose_plus":
        return _pack(*fx.pose_plus_exact(c["x"], c["delta"]))
    if family == "se3_plus":
        return _pack(*fx.se3_plus_exact(c["x"], c["delta"]))
    if family == "prior":
        groups, terms, ws = fx.prior_exact(c["J0"], c["r0"], c["blocks"], c["params"])
        out = _pack(groups, terms)
        out["ws"] = ws
        return out
    raise KeyError(family)


def err(got, ex):
    """max|got - exact| / scale for exact = hi + lo; got - hi is formed first, so the difference keeps the low part"""
    hi, lo, scale = ex
    got = np.ravel(got)
    assert got.shape == hi.shape, (got.shape, hi.shape)
    with np.errstate(invalid="ignore"):
        d = np.abs((got - hi) - lo)
    if not np.isfinite(d).all():
        return float("inf")
    m = float(d.max(initial=0.0))
    return 0.0 if m == 0.0 else m / scale if scale > 0 else float("inf")


def errors(outputs, ex):
    return {g: err(v, ex[g]) for g, v in outputs.items()}


def local(J):
    """a Ceres block of a pose (rows x 7) -> its six local columns; the 7th must be zero"""
    assert not J[:, 6].any()
    return J[:, :6]


def make_prior(c):
    return abi.make_prior(c["J0"], c["r0"], c["blocks"])


def lidar_constraint(c):
    lc = abi.LidarConstraint()
    lc.q[:] = list(c["q"]); lc.t[:] = list(c["t"])
    return lc


def proj_outputs(r, J, td=False):
    out = {"residual": r, "J_pose_i": local(J[0]), "J_pose_j": local(J[1]), "J_ex_pose": local(J[2]), "J_feature": J[3]}
    if td:
        out["J_td"] = J[4]
    return out


def td_args(c):
    return (c["params"], c["pts_i"], c["pts_j"], c["vel_i"], c["vel_j"], float(c["td_i"]), float(c["td_j"]), float(c["row_i"]), float(c["row_j"]))


def as_td(c):
    """a projection case as the call of the general routine that computes the same: zero velocities, td = td_i = td_j = 0"""
    return (c["params"] + [np.zeros(1)], c["pts_i"], c["pts_j"], np.zeros(2), np.zeros(2), 0.0, 0.0, 0.0, 0.0)


# ---- what the oracle gives (CPU; also the yardstick of the GPU tests) --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_outputs(family, name):
    import oracle_lib as O
    c = cases(family)[name]
    L = O.lib()
    if family == "projection":
        r, J = O.eval_factor("projection", sets()[c["opt"]], c["params"], c["pts_i"], c["pts_j"], sizes=[7, 7, 7, 1], nres=2)
        return proj_outputs(r, J)
    if family == "projection_td":
        r, J = O.eval_factor("projection_td", sets()[c["opt"]], *td_args(c), sizes=[7, 7, 7, 1, 1], nres=2)
        return proj_outputs(r, J, td=True)
    if family == "lidar":
        r, J = O.eval_factor("lidar_between", sets()[c["opt"]], c["params"], lidar_constraint(c), sizes=[7, 7], nres=6)
        return {"residual": r, "J_pose_i": local(J[0]), "J_pose_j": local(J[1])}
    f = lambda v: abi.dptr(np.ascontiguousarray(v, dtype=np.float64))
    if family == "edge":
        r = np.zeros(3); J = np.zeros((3, 7))
        L.vilo_eval_edge(f(c["pose"]), f(c["cp"]), f(c["a"]), f(c["b"]), abi.dptr(r), abi.dptr(J))
        return {"residual": r, "J": local(J)}
    if family == "surf":
        r = np.zeros(1); J = np.zeros((1, 7))
        L.vilo_eval_surf.argtypes = [abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_double, abi.c_double_p, abi.c_double_p]
        L.vilo_eval_surf(f(c["pose"]), f(c["cp"]), f(c["n"]), float(c["d"]), abi.dptr(r), abi.dptr(J))
        return {"residual": r, "J": local(J)}
    if family == "pose_plus":
        o = np.zeros(7)
        L.vilo_pose_plus(f(c["x"]), f(c["delta"]), abi.dptr(o))
        return {"p": o[:3], "q": o[3:]}
    if family == "se3_plus":
        o = np.zeros(7)
        L.vilo_se3_plus(f(c["x"]), f(c["delta"]), abi.dptr(o))
        return {"q": o[:4], "t": o[4:]}
    if family == "prior":
        r, J = O.eval_factor("prior", None, c["params"], make_prior(c), sizes=[b["size"] for b in c["blocks"]], nres=c["n"])
        return {"residual": r, "jacobians": J}
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def oracle_errors(family, name):
    out = oracle_outputs(family, name)
    ex = exact(family, name)
    return {g: err(v, ex[g]) for g, v in out.items() if g in ex}


# ---- bounds that are not CPU_BOUND ----------------------------------------------------------------------------------------------------------
def prior_row_bound(c):
    """r = r0 + J0 dx, a dot product of n + 1 terms per row: (n + 16) eps (|r0| + |J0| |dx|) row by row covers the n additions, the products and the few eps
    that dx itself carries (a difference, or the vector part of a quaternion product)"""
    ex = exact("prior", c_name(c))
    dx = np.abs(ex["dx"][0])
    return (c["n"] + 16) * EPS * (np.abs(c["r0"]) + np.abs(c["J0"]) @ dx)


def c_name(c):
    return next(k for k, v in cases("prior").items() if v is c)


def se3_translation_bound(c):
    """The reference's own (1 - cos t) / t^2 Omega carries the cosine's rounding: a cosine off by k units of 2^-53 moves 1 - cos t by as much, the factor by
    k 2^-53 / t^2 and the translation by at most k 2^-53 / t |upsilon|; (t - sin t) / t^3 Omega^2 adds at most k eps |upsilon|. One unit for each library's
    cosine, doubled as margin: (4 2^-53 / t + 16 eps)(|upsilon| + |t|), absolute. For t < 1e-10 the other branch runs and CPU_BOUND holds."""
    th = fx.se3_theta(c["delta"])
    size = float(np.linalg.norm(c["delta"][3:]) + np.linalg.norm(c["x"][4:]))
    return (4.0 * 2.0 ** -53 / th + 16.0 * EPS) * size


def within(dev, ref, what):
    """device errors against the oracle's on the same case and group: 4 x + 16 eps of the scale"""
    bad = {g: (dev[g], ref[g]) for g in dev if not dev[g] <= FACTOR * ref[g] + FLOOR}
    assert not bad, (what, bad)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_case_list_holds_what_it_claims():
    """The property that makes each case an edge, proved on the exact values."""
    S = sets()
    f = lambda g: np.asarray(g[0])
    # option sets: the branch of Quaterniond(RIC RCL) and the norm of qil
    branch, qnorm = {}, {}
    for name in fc.OPTION_NAMES:
        o = S[name]
        qil, _, br = fx.lidar_extrinsic_exact(o.RIC[:], o.TIC[:], o.RCL[:], o.TCL[:])
        branch[name] = br
        qnorm[name] = float(fx.mp.sqrt(sum(x.v * x.v for x in qil)))
    assert branch == {"default": 3, "alt": 3, "alt7": 3, "br0": 0, "br1": 1, "br2": 2}, branch
    assert abs(qnorm["alt"] - 1.0) < 4 * EPS and 3e-8 < abs(qnorm["alt7"] - 1.0) < 3e-7, qnorm
    ric = np.array(S["alt"].RIC[:]).reshape(3, 3)
    assert np.abs(ric).max() < 0.97 and np.abs(ric).min() > 0.02, "a general RIC: no entry near 0 or 1"
    # projection
    P = cases("projection")
    assert np.abs(P["far_5km"]["params"][0][:3]).min() >= 2990 and 0.49 < np.linalg.norm(P["far_5km"]["params"][0][:3] - P["far_5km"]["params"][1][:3]) < 0.51
    assert [P[n]["params"][3][0] for n in ("inv_dep_2", "inv_dep_1e-3", "inv_dep_1e-6", "inv_dep_negative")] == [2.0, 1e-3, 1e-6, -0.2]
    assert f(exact("projection", "inv_dep_negative")["pts_camera_j"])[2] < 0, "the point is behind camera j: the reference has no guard"
    assert np.array_equal(P["same_pose"]["params"][0], P["same_pose"]["params"][1])
    z = f(exact("projection", "low_z")["pts_camera_j"])[2]; depth = 1.0 / P["low_z"]["params"][3][0]
    assert 0 < z < 0.3 * depth, (z, depth)                                    # z = 2.10 of a depth of 10
    for n, which in (("neg_Qi", (0,)), ("neg_Qj", (1,)), ("neg_qic", (2,)), ("neg_all", (0, 1, 2))):
        for k in range(3):
            want = -P["plain0"]["params"][k][3:] if k in which else P["plain0"]["params"][k][3:]
            assert np.array_equal(P[n]["params"][k][3:], want), (n, k)
    # projection with td
    T = cases("projection_td")
    for opt in ("default", "alt"):
        ROW = float(S[opt].ROW)
        assert T["row_0_" + opt]["row_i"] == 0.0 and T["row_last_" + opt]["row_i"] == ROW - 1 and T["row_half_" + opt]["row_i"] == ROW / 2
        assert not T["velocity_zero_at_i_" + opt]["vel_i"].any() and T["velocity_zero_at_i_" + opt]["vel_j"].all()
        assert not T["velocity_zero_at_j_" + opt]["vel_j"].any() and T["velocity_zero_at_j_" + opt]["vel_i"].all()
        assert np.abs(T["plain_" + opt]["vel_i"]).tolist() == [2.0, 1.5]
    assert S["default"].TR == 0.0 and S["alt"].TR == 0.033 and S["alt"].ROW == 375.0 and S["alt"].focal_length == 718.856
    d = T["degenerate_default"]
    assert d["params"][4][0] == d["td_i"] == d["td_j"] and d["vel_i"].all()
    # lidar
    Lc = cases("lidar")
    assert np.array_equal(Lc["same_pose_identity"]["params"][0], Lc["same_pose_identity"]["params"][1]) and Lc["same_pose_identity"]["q"][3] == 1.0
    assert Lc["lidar_q_negative_w"]["q"][3] < 0 and np.abs(Lc["far_5km"]["params"][0][:3]).min() >= 2990
    assert np.isclose(np.linalg.norm(Lc["translation_30m"]["t"]), 30.0, rtol=1e-12)
    rq = f(exact("lidar", "residual_3rad")["residual"])[3:] / 100.0           # 2 vec(q): |.| = 2 sin(1.5) = 1.99499
    assert 1.99 < np.linalg.norm(rq) < 2.0, np.linalg.norm(rq)
    assert sorted(n[:-2] for n in Lc if n[-2] == "_" and n[:-2] in fc.OPTION_NAMES) == sorted(["alt", "alt7", "br0", "br1", "br2"] * 2)
    # edge / surf
    Ec = cases("edge")
    nab = lambda c: float(np.linalg.norm(c["a"] - c["b"]))
    assert np.isclose(nab(Ec["ab_1e-3"]), 1e-3, rtol=1e-9) and np.isclose(nab(Ec["ab_50"]), 50.0, rtol=1e-12)
    assert np.isclose(np.linalg.norm(Ec["cp_80m_1rad"]["cp"]), 80.0, rtol=1e-12) and abs(Ec["cp_80m_1rad"]["pose"][3] - fc.COS_HALF[1.0]) < 1e-15
    assert np.abs(f(exact("edge", "point_on_line")["residual"])).max() < 1e-13, "on the line to the rounding of cp"
    assert np.abs(Ec["ab_5km"]["a"]).min() >= 2990
    sr = float(f(exact("surf", "cancels_to_1e-9")["residual"])[0]); sc = cases("surf")["cancels_to_1e-9"]
    assert 0.9e-9 < sr < 1.1e-9 and 99.0 < abs(sc["d"]) < 101.0, (sr, sc["d"])
    # Plus
    Pp = cases("pose_plus")
    assert not Pp["dtheta_0"]["delta"][3:].any() and np.isclose(np.linalg.norm(Pp["dtheta_1e-12"]["delta"][3:]), 1e-12, rtol=1e-12, atol=0.0)
    assert np.isclose(np.linalg.norm(Pp["dtheta_3"]["delta"][3:]), 3.0) and Pp["negative_w"]["x"][6] < 0 and np.abs(Pp["far_5km"]["x"][:3]).min() >= 2990
    Sp = cases("se3_plus")
    assert len(Sp) == 2 * len(fc.SE3_THETAS)
    for c in Sp.values():
        th = fx.se3_theta(c["delta"])
        assert abs(th - c["theta"]) <= 4 * EPS * c["theta"] and (th < 1e-10) == (c["theta"] in (0.0, 1e-12, 9e-11)), (c["theta"], th)
        assert np.isclose(np.linalg.norm(c["x"][4:]), 100.0) and np.isclose(np.linalg.norm(c["delta"][3:]), c["upsilon"])
    # prior
    Pr = cases("prior")
    for b, x in zip(Pr["x_equals_x0"]["blocks"], Pr["x_equals_x0"]["params"]):
        assert np.array_equal(b["x0"], x)
        if b["size"] == 7:
            q = b["x0"][3:]
            assert q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] == 1.0 and np.array_equal(q * 4, np.round(q * 4)), "products of the components are exact"
    assert not np.abs(f(exact("prior", "x_equals_x0")["dx"])).any()
    ws = lambda n: np.array([float(w) for w in exact("prior", n)["ws"].values()])
    assert (ws("negated_quaternions") < 0).all() and (ws("negated_quaternions_base") > 0).all() and len(ws("negated_quaternions")) == 12
    assert np.allclose(ws("w_plus_1e-3"), 1e-3, rtol=1e-9) and np.allclose(ws("w_minus_1e-3"), -1e-3, rtol=1e-9)      # 179.885 and 180.115 degrees
    assert Pr["n_157"]["n"] == 157 and len(Pr["n_157"]["blocks"]) == 22 and sorted({b["size"] for b in Pr["n_157"]["blocks"]}) == [1, 7, 9]
    assert Pr["n_1"]["n"] == 1 and [b["size"] for b in Pr["n_1"]["blocks"]] == [1]
    a = np.abs(Pr["J0_1e-6_to_1e6"]["J0"])
    assert a.min() < 1e-6 and a.max() > 1e5


@pytest.mark.parametrize("family", ["projection", "projection_td", "lidar", "edge", "surf", "pose_plus"])
def test_oracle_against_exact(oracle, family):
    """Every case, every group, within 64 eps of the scale (CPU_BOUND)."""
    for name in cases(family):
        e = oracle_errors(family, name)
        bad = {g: v for g, v in e.items() if not v <= CPU_BOUND}
        assert not bad, (family, name, bad)


def test_oracle_se3_plus_against_exact(oracle):
    """The rotation within CPU_BOUND everywhere; the translation within CPU_BOUND below the 1e-10 threshold and within se3_translation_bound above it. No test inside
    the band 1e-10 <= theta < 1e-8 can tell the threshold from 1e-8: there (1 - cos theta) is 0 or a few units of 2^-53, and the bound is as large as the term."""
    for name, c in cases("se3_plus").items():
        e = oracle_errors("se3_plus", name)
        ex = exact("se3_plus", name)
        assert e["q"] <= CPU_BOUND, (name, e)
        if fx.se3_theta(c["delta"]) < 1e-10:
            assert e["t"] <= CPU_BOUND, (name, e)
        else:
            assert e["t"] * ex["t"][2] <= se3_translation_bound(c), (name, e["t"] * ex["t"][2], se3_translation_bound(c))


def test_oracle_prior_against_exact(oracle):
    """Residual within the dot-product bound row by row; the Jacobian blocks are J0's columns to the bit; x = x0 gives r0 to the bit."""
    for name, c in cases("prior").items():
        out = oracle_outputs("prior", name)
        check_prior(out["residual"], out["jacobians"], name, c)


def check_prior(r, J, name, c):
    hi, lo, _ = exact("prior", name)["residual"]
    d = np.abs((r - hi) - lo)
    assert (d <= prior_row_bound(c)).all(), (name, float((d / prior_row_bound(c)).max()))
    for b, Jb in zip(c["blocks"], J):
        ls = 6 if b["size"] == 7 else b["size"]
        assert np.array_equal(Jb[:, :ls], c["J0"][:, b["idx"]:b["idx"] + ls]) and not Jb[:, ls:].any(), (name, b["id"])
    if name == "x_equals_x0":
        assert np.array_equal(r, c["r0"]), name


def negated_prior(prior):
    p = copy.copy(prior)
    for i in range(p.n_blocks):
        if p.block_size[i] == 7:
            for k in range(3, 7):
                p.block_x0[i][k] = -p.block_x0[i][k]
    return p


RESULT_ARRAYS = ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature", "para_pose", "para_speed_bias", "tic", "ric")
RESULT_SUMMARY = ("num_iterations", "num_successful_steps", "num_linear_solves", "termination", "initial_cost", "final_cost", "final_radius")


def assert_same_bits(a, b, what):
    for key in RESULT_ARRAYS:
        assert np.array_equal(getattr(a, key), getattr(b, key)), (what, key)
    assert a.td == b.td
    for key in RESULT_SUMMARY:
        assert a.summary[key] == b.summary[key], (what, key)


def prior_bytes(p):
    J, r, blocks = abi.prior_to_numpy(p)
    return J, r, [(b["id"], b["size"], b["idx"]) for b in blocks], np.concatenate([b["x0"] for b in blocks])


def assert_same_prior(a, b, what):
    assert a.valid == b.valid and a.n == b.n and a.m == b.m and a.n_blocks == b.n_blocks, what
    for x, y in zip(prior_bytes(a), prior_bytes(b)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, what


def test_oracle_window_prior_sign_branch(oracle, opts):
    """A prior whose x0 quaternions all changed sign: q_inv and q_mul of a negated quaternion are the exact negatives and the sign flip of w < 0 undoes them, so dx
    is the same bits and with it the whole solve and the prior the marginalization leaves. Without the flip the rotation part of dx changes sign and the solve differs."""
    win, prior, _ = synth.make_window(41, opts, synth.SynthConfig(with_prior=True))
    neg = negated_prior(prior)
    assert sum(prior.block_size[i] == 7 for i in range(prior.n_blocks)) >= 2
    a = oracle.window_solve(opts, win, prior); b = oracle.window_solve(opts, win, neg)
    assert_same_bits(a, b, "oracle solve")
    assert_same_prior(oracle.window_marginalize(opts, win, a, prior), oracle.window_marginalize(opts, win, b, neg), "oracle marginalization")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solvers():
    """one BackendSolver per option set, created on first use"""
    from vil_fusion_amd.estimator import BackendSolver
    made = {}

    def get(name):
        if name not in made:
            made[name] = BackendSolver(copy.copy(sets()[name]))          # raises VilfError when the HIP library / GPU is missing: no silent fallback
        return made[name]
    yield get
    for s in made.values():
        s.close()


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_device_projection_against_exact(solvers, oracle):
    """Every projection case through both device routines: vilf_eval_projection (blocks i, j and lambda from pair_table / projection_eval_pair, the Ex block from the
    general routine) and vilf_eval_projection_td with zero velocities (projection_td_eval, all blocks). A case with negated quaternions equals its base to the bit:
    the quaternions enter only through q_toR, which is quadratic."""
    got = {}
    for name, c in cases("projection").items():
        s = solvers(c["opt"])
        ex = exact("projection", name)
        r, J = s.eval_projection(c["params"], c["pts_i"], c["pts_j"])
        r2, J2 = s.eval_projection_td(*as_td(c))
        got[name] = [r] + J + [r2] + J2[:4]
        ref = oracle_errors("projection", name)
        pair, general = errors(proj_outputs(r, J), ex), errors(proj_outputs(r2, J2), ex)
        print("projection %-18s pair %s general %s oracle %s" % (name, _fmt(pair), _fmt(general), _fmt(ref)))
        within(pair, ref, ("pair table", name))
        within(general, ref, ("general routine", name))
        assert not J2[4].any(), "zero velocities: no dependence on td"
    for name, c in cases("projection").items():
        if "same_as" in c:
            assert same_bits(got[name], got[c["same_as"]]), (name, "differs from", c["same_as"])


def _fmt(e):
    return " ".join("%s=%.2g" % (g, v / EPS) for g, v in e.items())


@pytest.mark.gpu
def test_device_projection_td_against_exact(solvers, oracle):
    """vilf_eval_projection_td on the td cases of both option sets (TR 0 and TR 0.033 with ROW 375), five blocks; td = td_i = td_j with TR 0 equals the zero-velocity
    call to the bit in everything but J_td."""
    got = {}
    for name, c in cases("projection_td").items():
        r, J = solvers(c["opt"]).eval_projection_td(*td_args(c))
        got[name] = (r, J)
        dev, ref = errors(proj_outputs(r, J, td=True), exact("projection_td", name)), oracle_errors("projection_td", name)
        print("projection_td %-34s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, name)
    (r, J), (r0, J0) = got["degenerate_default"], got["degenerate_zero_velocity_default"]
    assert same_bits([r] + J[:4], [r0] + J0[:4]) and J[4].any() and not J0[4].any()


@pytest.mark.gpu
def test_device_lidar_between_against_exact(solvers, oracle):
    """vilf_eval_lidar_between on every case and option set: qil from all four branches of the host's quat_from_R, and a qil off unit norm by 1e-7 (alt7)."""
    for name, c in cases("lidar").items():
        r, J = solvers(c["opt"]).eval_lidar_between(c["params"], lidar_constraint(c))
        dev = errors({"residual": r, "J_pose_i": local(J[0]), "J_pose_j": local(J[1])}, exact("lidar", name))
        ref = oracle_errors("lidar", name)
        print("lidar %-22s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, name)


@pytest.mark.gpu
def test_device_edge_surf_against_exact(solvers, oracle):
    s = solvers("default")
    for name, c in cases("edge").items():
        r, J = s.eval_edge(c["pose"], c["cp"], c["a"], c["b"])
        dev, ref = errors({"residual": r, "J": local(J)}, exact("edge", name)), oracle_errors("edge", name)
        print("edge %-16s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, ("edge", name))
    for name, c in cases("surf").items():
        r, J = s.eval_surf(c["pose"], c["cp"], c["n"], c["d"])
        dev, ref = errors({"residual": r, "J": local(J)}, exact("surf", name)), oracle_errors("surf", name)
        print("surf %-16s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, ("surf", name))


@pytest.mark.gpu
def test_device_plus_against_exact(solvers, oracle):
    """pose_plus at 4 x the oracle's error + 16 eps; se3_plus the same for the rotation and below the threshold, and for the translation at theta >= 1e-10 the bound
    derived at se3_translation_bound for oracle and device alike (the two need not be within a factor of four of each other there)."""
    s = solvers("default")
    for name, c in cases("pose_plus").items():
        o = s.pose_plus(c["x"], c["delta"])
        dev, ref = errors({"p": o[:3], "q": o[3:]}, exact("pose_plus", name)), oracle_errors("pose_plus", name)
        print("pose_plus %-14s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, ("pose_plus", name))
    for name, c in cases("se3_plus").items():
        o = s.pose_plus(c["x"], c["delta"], se3=True)
        ex = exact("se3_plus", name)
        dev, ref = errors({"q": o[:4], "t": o[4:]}, ex), oracle_errors("se3_plus", name)
        print("se3_plus %-28s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        if fx.se3_theta(c["delta"]) < 1e-10:
            within(dev, ref, ("se3_plus", name))
        else:
            within({"q": dev["q"]}, ref, ("se3_plus", name))
            assert dev["t"] * ex["t"][2] <= se3_translation_bound(c), (name, dev["t"] * ex["t"][2], se3_translation_bound(c))


@pytest.mark.gpu
def test_device_prior_against_exact(solvers, oracle):
    """vilf_eval_prior on every prior case: the residual within the dot-product bound row by row and within 4 x the oracle's error + 16 eps as a group, the Jacobian
    blocks J0's columns to the bit, x = x0 gives r0 to the bit, and negated parameter quaternions give the bits of the un-negated ones (the w < 0 branch of k_hook_prior)."""
    s = solvers("default")
    got = {}
    for name, c in cases("prior").items():
        r, J = s.eval_prior(make_prior(c), c["params"])
        got[name] = r
        check_prior(r, J, name, c)
        dev, ref = {"residual": err(r, exact("prior", name)["residual"])}, oracle_errors("prior", name)
        print("prior %-26s device %s oracle %s" % (name, _fmt(dev), _fmt(ref)))
        within(dev, ref, name)
    assert np.array_equal(got["negated_quaternions"], got["negated_quaternions_base"])


@pytest.mark.gpu
def test_eval_prior_rejects_a_malformed_block_table(solvers, oracle):
    """vilf_eval_prior checks the block table as vilf_prior_import does, before anything is copied or launched: a size of 8, a negative idx and idx + local = n + 1 are
    VILF_ERR_INVALID_ARGUMENT (k_hook_prior indexes its LDS vector with the table); a valid call afterwards still agrees with the exact reference."""
    s = solvers("default")
    c = cases("prior")["small_step"]
    L = s._L
    for what, field, i, value in (("size 8", "block_size", 3, 8), ("negative idx", "block_idx", 2, -1), ("idx + local = n + 1", "block_idx", 12, c["n"] - 9 + 1)):
        p = make_prior(c)
        assert p.block_size[12] == 9 and p.block_idx[12] + 9 == c["n"]
        getattr(p, field)[i] = value
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in c["params"]]
        pp = (abi.c_double_p * len(arrs))(*[abi.dptr(a) for a in arrs])
        r = np.full(c["n"], np.nan)
        rc = L.vilf_eval_prior(s._h, C.byref(p), pp, abi.dptr(r), None)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and np.isnan(r).all(), (what, rc)
    r, J = s.eval_prior(make_prior(c), c["params"])
    check_prior(r, J, "small_step", c)


@pytest.mark.gpu
def test_window_prior_sign_branch_fixed_path(oracle, opts):
    """The prior's w < 0 branch in the product path (prior_setup of the window kernels, the marginalization): an 11-frame window solved and marginalized with a prior and
    with the same prior whose x0 quaternions changed sign. dx is the same bits (see test_oracle_window_prior_sign_branch), so every state, count and cost and the
    exported prior are bit-identical."""
    from vil_fusion_amd.estimator import BackendSolver
    win, prior, _ = synth.make_window(41, opts, synth.SynthConfig(with_prior=True))
    s = BackendSolver(opts)
    try:
        res, out = [], []
        for p in (prior, negated_prior(prior)):
            s.set_prior(p)
            res.append(s.optimization(win))
            s.marginalize()
            out.append(s.get_prior())
    finally:
        s.close()
    ref = oracle.window_solve(opts, win, prior)
    assert res[0].summary["num_iterations"] == ref.summary["num_iterations"] and np.abs(res[0].Ps - ref.Ps).max() < 1e-7
    assert_same_bits(res[0], res[1], "device solve")
    assert out[0].valid and out[0].n > 0
    assert_same_prior(out[0], out[1], "device marginalization")


def general_path_problem(oracle):
    """estimate_extrinsic = 1 with a prior on an 11-frame window, the extrinsic moved off its optimum: vilf_window_solve's general single-window path"""
    o = oracle.default_options()
    o.estimate_extrinsic = 1
    win, prior, _ = synth.make_window(81, o, synth.SynthConfig(n_frames=11, n_features=120, with_prior=True))
    rng = fc.rng_of(6)
    ex = win.para_ex_pose.copy()
    ex[:3] += fc.uni(rng, -0.01, 0.01, 3)
    ex[3:] = fc.unit(fc.qmul(ex[3:], fc.unit(np.concatenate([fc.uni(rng, -0.003, 0.003, 3), [1.0]]))))
    win.para_ex_pose = ex
    return o, win, prior


def test_oracle_general_problem_prior_sign_branch(oracle):
    """the oracle's solve of the general-path problem is bit-identical under the negated prior as well"""
    o, win, prior = general_path_problem(oracle)
    assert_same_bits(oracle.window_solve(o, win, prior), oracle.window_solve(o, win, negated_prior(prior)), "oracle, estimate_extrinsic")


@pytest.mark.gpu
def test_window_prior_sign_branch_general_path(oracle):
    """The same through the general single-window path (estimate_extrinsic = 1 with a prior; vilf_lw.hip:1287, :1665). This path is NOT bit-reproducible run to run:
    with estimate_extrinsic / estimate_td the kernels lw_visual_ext, lw_prior and lw_imu_lidar_prior add into Hpp and g_p with floating-point atomics from several
    workgroups in no fixed order (vilf_lw.hip, the comment at lw_acc), and two solves of the SAME prior already differ in the last bits. So bits cannot be asserted:
    the solve with the prior and the one with the negated prior are each compared with the oracle at the tolerances of test_extrinsic_and_td_estimation_match_oracle,
    with equal counts. A lost sign flip changes the sign of the rotation part of dx: the initial cost alone is then off by many orders more than 1e-9."""
    from vil_fusion_amd.estimator import BackendSolver
    o, win, prior = general_path_problem(oracle)
    s = BackendSolver(o)
    try:
        res = []
        for p in (prior, negated_prior(prior)):
            s.set_prior(p)
            res.append(s.optimization(win))
    finally:
        s.close()
    ref = oracle.window_solve(o, win, prior)
    assert np.abs(ref.tic - win.para_ex_pose[:3]).max() > 1e-5, "the extrinsic must have moved"
    for got, what in zip(res, ("prior", "negated prior")):
        for key in ("num_iterations", "num_successful_steps"):
            assert got.summary[key] == ref.summary[key], (what, key)
        assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"], what
        assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= 1e-6 * ref.summary["final_cost"], what
        assert np.abs(got.Ps - ref.Ps).max() < 1e-6 and np.abs(got.Rs - ref.Rs).max() < 1e-7 and np.abs(got.Vs - ref.Vs).max() < 1e-5, what
        assert np.abs(got.tic - ref.tic).max() < 1e-6 and np.abs(got.ric - ref.ric).max() < 1e-7 and abs(got.td - ref.td) < 1e-7, what
