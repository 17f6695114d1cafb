"""Designed inputs of the scan-to-map pose solve (b_solve) for tests/test_scan2map_solve.py: factor records per query slot, seeded and small.

Every case draws its factors from a POOL of at most 64 distinct ones (a scene: scan points 2 .. 15 m out, lines and planes of the world through their images under a
true pose, a start pose some way off), laid out over the query slots with a multiplicity each, so that the exact tier evaluates at most 64 factors per sweep whatever
the slot count. Slots without a factor (kind 0, and kind 3, the tie marker) are interleaved: every seventh slot, the slot at each multiple of 256 and the last slot
unless the case says otherwise; they carry a real factor's record, so that a sweep that ignores the kind shows.

exact_* cases sit on a threshold and are built from dyadic numbers at the identity pose, where the operations that lead to the threshold quantity are exact in fp64:
  exact_huber_on / exact_huber_above   planes n = +-e_k, d and scan points multiples of 2^-3 (the 'above' case: one offset 2^-20 more), one line along x with
        |pa - pb| = 1/4: q = (0,0,0,1) and t = 0 make q * cp + t = cp (products by 0 and 1, sums with 0); r = n . cp + d, the cross product of the edge, the division by
        1/4 and s = |r|^2 (2^-6, or 2^-6 + 2^-22 + 2^-40: 35 bits) are sums and products of dyadic numbers with no rounding. At s = a^2 both branches of Huber's rule
        give rho0 = a^2 and weight 1 — the switch itself is not observable there — and 2^-20 beyond it the outer branch is.
  exact_small_angle   every scan point at the origin, identity start: lp = 0, the rotational jacobian -(n x lp) is a product with 0 in every entry, so the rotational
        gradient, the rotational rows of H and (0 / pivot) the rotational step are exactly 0: the diagonal there is the 1e-6 clamp and Plus takes its theta < 1e-10 branch.
  exact_min   planes +-e_k through their own scan points: r = 0 exactly, cost 0, g = 0: the gradient stop before any iteration.
  c_1_0 / c_0_1   one axis-aligned factor: rows of exact zeros rest on the clamp."""
import functools
import numpy as np

F32 = np.float32
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
CAP_EDGE, CAP_SURF = 70016, 65600          # scan capacities of the test batch (three streams)
TRACE_ROWS = 52


def _quat(axis, ang):
    axis = np.asarray(axis, dtype=np.float64); axis = axis / np.linalg.norm(axis)
    return np.append(np.sin(ang / 2) * axis, np.cos(ang / 2))


def _rot(q, v):
    qv, w = q[:3], q[3]
    uv = 2 * np.cross(qv, v)
    return v + w * uv + np.cross(qv, uv)


def pool(seed, n_edge=24, n_surf=24, noise=0.02, true_pose=None, outliers=0, out_size=0.5):
    """distinct factors of a scene -> (kind [P], rec [P, 6], cp float32 [P, 3])"""
    rng = np.random.default_rng(seed)
    tp = np.concatenate([_quat([0.2, -0.4, 1.0], 0.3), [1.5, -0.7, 0.3]]) if true_pose is None else np.asarray(true_pose, dtype=np.float64)
    P = n_edge + n_surf
    cp = (rng.uniform(2, 15, (P, 1)) * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(P, 3)))).astype(F32)
    kind = np.array([1] * n_edge + [2] * n_surf, dtype=np.int32)
    rec = np.zeros((P, 6))
    for i in range(P):
        w = _rot(tp[:4], cp[i].astype(np.float64)) + tp[4:]
        e = rng.normal(0, noise, 3)
        if i % max(P // max(outliers, 1), 1) == 0 and outliers:
            e = e + out_size * rng.normal(size=3)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        if kind[i] == 1:
            c = w + e - d * np.dot(e, d)
            rec[i, :3] = c + 0.1 * d; rec[i, 3:] = c - 0.1 * d
        else:
            rec[i, :3] = d; rec[i, 3] = -np.dot(d, w) + e[0]
    return kind, rec, cp


def layout(pl, n_edge_q, n_surf_q, invalid="std", n_valid=None, last_valid=False):
    """slots from a pool -> kind_slot [nq], idx_slot [nq] (pool index of the record the slot carries)"""
    kind_p = pl[0]
    pe, ps = np.nonzero(kind_p == 1)[0], np.nonzero(kind_p == 2)[0]
    nq = n_edge_q + n_surf_q
    i = np.arange(nq)
    is_e = i < n_edge_q
    idx = np.where(is_e, pe[i % len(pe)] if len(pe) else 0, ps[(i - n_edge_q) % len(ps)] if len(ps) else 0)
    kind = np.where(is_e, 1, 2).astype(np.int32)
    if invalid == "std":
        bad = (i % 7 == 3) | (i % 256 == 0)
        if nq:
            bad[-1] = True
    elif invalid == "all":
        bad = np.ones(nq, dtype=bool)
    else:
        bad = np.zeros(nq, dtype=bool)
    if last_valid and nq:
        bad[-1] = False
    if n_valid is not None:                      # exactly n_valid factors: flip slots from the front, never the last one
        have = int((~bad).sum())
        pos = np.nonzero(bad[:-1] if have < n_valid else ~bad[:-1])[0][:abs(n_valid - have)]
        bad[pos] = have >= n_valid
        assert int((~bad).sum()) == n_valid
    kind[bad] = np.where(i[bad] % 2 == 0, 0, 3)
    return kind, idx


def make(name, pl, n_edge_q, n_surf_q, pose, huber_a=0.1, max_it=4, stream=2, target=None, **lay):
    kind_p, rec_p, cp_p = pl
    kind, idx = layout(pl, n_edge_q, n_surf_q, **lay)
    valid = (kind == 1) | (kind == 2)
    vi = idx[valid]
    used, mult = np.unique(vi, return_counts=True) if len(vi) else (np.zeros(0, dtype=int), np.zeros(0, dtype=int))
    c = dict(name=name, n_edge_q=n_edge_q, n_surf_q=n_surf_q, pose=np.asarray(pose, dtype=np.float64), huber_a=huber_a, max_it=max_it, stream=stream,
             kind_slot=np.ascontiguousarray(kind), rec_slot=np.ascontiguousarray(rec_p[idx]) if len(idx) else np.zeros((0, 6)),
             cp_slot=np.ascontiguousarray(cp_p[idx]) if len(idx) else np.zeros((0, 3), dtype=F32),
             n_valid=int(valid.sum()), nfe=int((kind == 1).sum()), nfs=int((kind == 2).sum()), target=target or {}, exact_huber=name.startswith("exact_huber"))
    c["f64"] = dict(kind=kind[valid], rec=rec_p[vi], cp=cp_p[vi].astype(np.float64), mult=np.ones(len(vi), dtype=int))
    c["mp_src"] = dict(kind=kind_p[used], rec=rec_p[used], cp=cp_p[used].astype(np.float64), mult=mult)
    assert len(used) <= 64
    return c


def _axis_pool(rows):
    """rows of (kind, rec6, cp3) given literally"""
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.float64), np.array([r[2] for r in rows], dtype=F32))


START = np.concatenate([_quat([1.0, 0.3, -0.2], 0.25), [1.3, -0.6, 0.45]])          # some 0.1 rad and 0.3 m from the scene's true pose


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    P = pool(11)
    # ---- counts
    cs.append(make("c_0_0", P, 0, 0, START, target=dict(its=0)))
    cs.append(make("c_all_invalid", P, 40, 40, START, invalid="all", target=dict(its=0)))
    e1 = _axis_pool([(1, [0.125, 0, 1, -0.125, 0, 1], [0.5, 0.25, 0.75])])
    s1 = _axis_pool([(2, [0, 0, 1, -0.25, 0, 0], [0.5, 0.25, 0.0])])
    # (one factor drives its cost to 0 in two or three iterations; behind that every stop test sits at 0 against 0 and is decided by nothing: the budget ends them before)
    cs.append(make("c_1_0", e1, 1, 0, IDENT, invalid="none", max_it=2, target=dict(clamped=1)))
    cs.append(make("c_0_1", s1, 0, 1, IDENT, invalid="none", max_it=1, target=dict(clamped=3)))
    for ne, ns in [(255, 0), (256, 0), (257, 0), (1, 300), (255, 257), (257, 255), (300, 1), (0, 511), (0, 513)]:
        cs.append(make(f"c_{ne}_{ns}", P, ne, ns, START))
    # ---- list limits (S2M_LCAP = 16384 listed slots; 16-bit slot numbers)
    cs.append(make("l_16384", P, 9000, 10200, START, n_valid=16384, target=dict(n_valid=16384)))
    cs.append(make("l_16385", P, 9000, 10200, START, n_valid=16385, target=dict(n_valid=16385)))
    cs.append(make("l_nfac_65535_last", P, 20000, 45535, START, n_valid=12000, last_valid=True, target=dict(nfac=65535, last_valid=True)))
    cs.append(make("l_nfac_65536", P, 20000, 45536, START, n_valid=12000, last_valid=True, target=dict(nfac=65536)))
    cs.append(make("l_33000_planes", P, 0, 33000, START, invalid="none", target=dict(nfs=33000)))
    cs.append(make("l_70000_edges", P, 70000, 0, START, invalid="none", target=dict(nfe=70000)))
    # ---- loop
    for m in (0, 1, 4, 50):
        cs.append(make(f"g_it{m}", P, 120, 200, START, max_it=m, target=dict(why="budget" if m < 4 else "function")))
    # a noise-free scene 30 m out: the steps shrink quadratically, and |x| = 36 makes the parameter tolerance wide enough to be met before the gradient stop
    tp30 = np.concatenate([_quat([0.2, -0.4, 1.0], 0.3), [30.0, -18.0, 6.0]])
    st30 = np.concatenate([_quat([0.2, -0.4, 1.0], 0.32), [30.05, -18.03, 6.02]])
    cs.append(make("g_parameter_stop", pool(6, noise=0.0, true_pose=tp30), 60, 90, st30, max_it=50, target=dict(why="parameter")))
    # found by a random search on the CPU (start rotations of 2 .. pi about random axes): eight planes, Huber idle, the second step overshoots and is rejected
    # three times (radius / 2, / 4, / 8 on the reused diagonal) before the fourth try is accepted
    big = np.concatenate([_quat([0.07559361074288512, -1.4267738509897323, -0.13504510003701392], 2.640944300140441), [0.0, 0.0, 0.0]])
    cs.append(make("g_reject_then_accept", pool(873, n_edge=1, n_surf=8), 0, 8, big, huber_a=10.0, max_it=12, invalid="none", target=dict(reject_then_accept=True)))
    ax = [(2, [1, 0, 0, -2.5, 0, 0], [2.5, 1, 0.5]), (2, [0, 1, 0, 1.25, 0, 0], [3, -1.25, 2]), (2, [0, 0, 1, -0.75, 0, 0], [-1, 2, 0.75]),
          (2, [-1, 0, 0, -4, 0, 0], [-4, 0.5, 1]), (2, [0, -1, 0, 2, 0, 0], [1, 2, -3]), (2, [0, 0, -1, 1.5, 0, 0], [0.25, -2, 1.5])]
    cs.append(make("exact_min", _axis_pool(ax), 0, 6, IDENT, invalid="none", max_it=4, target=dict(why="gradient", its=0)))
    # ---- small angle and clamp
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=(9, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    sa = [(2, [n[0], n[1], n[2], d, 0, 0], [0, 0, 0]) for n, d in zip(nrm, rng.uniform(-0.3, 0.3, 9))]
    cs.append(make("exact_small_angle", _axis_pool(sa), 0, 9, IDENT, invalid="none", max_it=1, target=dict(small=True, clamped=3)))
    # ---- Huber switch, a = 1/8
    hub = [(2, [0, 0, 1, -0.5 + 0.125, 0, 0], [1, 2, 0.5]), (2, [0, 1, 0, 1.25 - 0.125, 0, 0], [3, -1.25, 2]), (2, [-1, 0, 0, -4 + 0.125, 0, 0], [-4, 0.5, 1]),
           (1, [0.125, 0, 0, -0.125, 0, 0], [0.5, 0.125, 0])]
    cs.append(make("exact_huber_on", _axis_pool(hub), 1, 3, IDENT, huber_a=0.125, invalid="none", max_it=0, target=dict(outer=0)))
    e = 2.0 ** -20
    hub2 = [(2, [0, 0, 1, -0.5 + 0.125 + e, 0, 0], [1, 2, 0.5]), (2, [0, 1, 0, 1.25 - 0.125 - e, 0, 0], [3, -1.25, 2]), (2, [-1, 0, 0, -4 + 0.125 + e, 0, 0], [-4, 0.5, 1]),
            (1, [0.125, 0, 0, -0.125, 0, 0], [0.5, 0.125 + e, 0])]
    cs.append(make("exact_huber_above", _axis_pool(hub2), 1, 3, IDENT, huber_a=0.125, invalid="none", max_it=1, target=dict(outer=4)))
    # ---- pose
    neg = START.copy(); neg[:4] = -neg[:4]
    cs.append(make("p_w_negative", P, 100, 140, neg, target=dict(w_negative=True)))
    far_true = np.concatenate([_quat([0.2, -0.4, 1.0], 0.3), [311.5, -204.7, 52.3]])
    # (close to the truth and two iterations: the rotation-translation coupling of a lever arm of 370 m makes the forward bounds grow a thousandfold per iteration)
    far_start = np.concatenate([_quat([0.2, -0.4, 1.0], 0.31), far_true[4:] + np.array([0.05, -0.025, 0.05 / 3])])
    cs.append(make("p_far", pool(13, true_pose=far_true), 100, 140, far_start, max_it=2, target=dict(far=True)))
    # ---- the single-stream context
    cs.append(make("single_stream", P, 130, 260, START, stream=-1))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs
