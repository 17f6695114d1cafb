"""Exact reference of the marginalization (MarginalizationInfo::marginalize, marginalization_factor.cpp:174-297) for tests/test_marginalization.py. CPU only.

The factor rows (residuals, Jacobians) come from the oracle's factor hooks at a given solved state, as in test_oracle_solver.test_marginalization_schur_vs_numpy;
everything behind the rows is exact or 60-digit arithmetic:
  * A = sum J^T J and b = sum J^T r in integer arithmetic (a double is an integer times a power of two: no rounding at all);
  * the elimination of the dropped blocks in mpmath, the features first (1-dimensional, mutually uncoupled: only the rows of a feature's own arrow are touched);
  * the reference's 1e-8 truncation decided on exact eigenvalues (mpmath.eigsy) wherever double precision cannot tell on which side of the cut an eigenvalue lies.
Nothing here looks at the device or at the oracle's marginalization."""
import math
import numpy as np
import mpmath as mp
from vil_fusion_amd import abi
import oracle_lib

DPS = 60
EPS_CUT = 1e-8                     # marginalization_factor.cpp:267, :283
BAND = (1e-9, 1e-7)                # no eigenvalue of a well-chosen case lies here: a decade on either side of the cut


class BadCase(AssertionError):
    """the case puts an eigenvalue next to the 1e-8 cut (or an Amm that is neither regular nor exactly singular): choose another case"""


def state_blocks(opts, win, state):
    """vector2double() of the solved state (estimator.cpp:505-547): para_Pose, para_SpeedBias, para_Ex_Pose, para_Td, para_Feature"""
    NF = win.n_frames
    L = oracle_lib.lib()
    pose = np.zeros((NF, 7)); sb = np.zeros((NF, 9)); q = np.zeros(4)
    for i in range(NF):
        L.vilo_quat_from_R(abi.dptr(np.ascontiguousarray(state.Rs[i])), abi.dptr(q))
        pose[i] = np.concatenate([state.Ps[i], q])
        sb[i] = np.concatenate([state.Vs[i], state.Bas[i], state.Bgs[i]])
    L.vilo_quat_from_R(abi.dptr(np.ascontiguousarray(state.ric, dtype=np.float64)), abi.dptr(q))
    ex = np.concatenate([state.tic, q])
    td = np.array([float(state.td)])
    with np.errstate(divide="ignore"):
        est = 1.0 / state.para_feature
    feat = np.where(est > 0, 1.0 / est, 1.0 / opts.init_depth)           # setDepth + getDepthVector (feature_manager.cpp:150-168, :194-216)
    return pose, sb, ex, td, feat


def factor_rows(opts, win, prior, state):
    """[(ids, sizes, r, [J per block])] of the factors that touch a dropped block, dropped ids, address shift {id: new id}, x0 per id"""
    NF = win.n_frames; W = NF - 1
    pose, sb, ex, td, feat = state_blocks(opts, win, state)
    ID_EX, ID_TD, ID_F = 2 * NF, 2 * NF + 1, 2 * NF + 2

    def blk(i):
        if i < NF: return pose[i]
        if i < 2 * NF: return sb[i - NF]
        if i == ID_EX: return ex
        if i == ID_TD: return td
        return feat[i - ID_F:i - ID_F + 1]
    factors = []; dropped = set(); shift = {}
    have_prior = prior is not None and prior.valid
    if have_prior:
        _, _, pblocks = abi.prior_to_numpy(prior)
        pids = [b["id"] for b in pblocks]; psz = [b["size"] for b in pblocks]
    if win.marginalization_flag == abi.MARGIN_OLD:
        if have_prior:
            r, J = oracle_lib.eval_factor("prior", None, [blk(i) for i in pids], prior, sizes=psz, nres=prior.n)
            factors.append((pids, psz, r, J))
            dropped |= {i for i in pids if i in (0, NF)}
        if opts.use_lidar_const:                                         # estimator.cpp:886-895, drop_set {0, 1}: Pose[1] leaves with Pose[0]
            c = abi.LidarConstraint.from_buffer_copy(win.lidar[1].tobytes())
            r, J = oracle_lib.eval_factor("lidar_between", opts, [pose[0], pose[1]], c, sizes=[7, 7], nres=6)
            factors.append(([0, 1], [7, 7], r, J)); dropped |= {0, 1}
        if win.imu[1, 0] < 10.0:                                         # :896-905
            pre = abi.ImuPreint.from_buffer_copy(win.imu[1].tobytes())
            r, J = oracle_lib.eval_factor("imu", opts, [pose[0], sb[0], pose[1], sb[1]], pre, sizes=[7, 9, 7, 9], nres=15)
            factors.append(([0, NF, 1, NF + 1], [7, 9, 7, 9], r, J)); dropped |= {0, NF}
        a2 = opts.cauchy_a * opts.cauchy_a
        for k in range(win.n_features):                                  # :907-950
            if win.feature_start_frame[k] != 0:
                continue
            o0, o1 = int(win.feature_obs_offset[k]), int(win.feature_obs_offset[k + 1])
            for t in range(o0 + 1, o1):
                j = t - o0
                if opts.estimate_td:
                    ids, sizes = [0, j, ID_EX, ID_F + k, ID_TD], [7, 7, 7, 1, 1]
                    r, J = oracle_lib.eval_factor("projection_td", opts, [pose[0], pose[j], ex, feat[k:k + 1], td], win.obs_point[o0], win.obs_point[t],
                                                  win.obs_velocity[o0], win.obs_velocity[t], float(win.obs_cur_td[o0]), float(win.obs_cur_td[t]),
                                                  float(win.obs_row[o0]), float(win.obs_row[t]), sizes=sizes, nres=2)
                else:
                    ids, sizes = [0, j, ID_EX, ID_F + k], [7, 7, 7, 1]
                    r, J = oracle_lib.eval_factor("projection", opts, [pose[0], pose[j], ex, feat[k:k + 1]], win.obs_point[o0], win.obs_point[t], sizes=sizes, nres=2)
                w = math.sqrt(1.0 / (1.0 + (r @ r) / a2))                  # Cauchy: rho'' < 0, the corrector is the plain sqrt(rho') scaling
                factors.append((ids, sizes, r * w, [Jb * w for Jb in J])); dropped |= {0, ID_F + k}
        for i in range(1, NF):
            shift[i] = i - 1; shift[NF + i] = NF + i - 1                 # :960-971
    else:
        if not have_prior or (W - 1) not in pids:
            return None                                                  # :982-983: the prior stays as it is
        r, J = oracle_lib.eval_factor("prior", None, [blk(i) for i in pids], prior, sizes=psz, nres=prior.n)
        factors.append((pids, psz, r, J)); dropped.add(W - 1)
        for i in range(NF):                                              # :1016-1037
            if i != W - 1:
                shift[i] = i - 1 if i == W else i; shift[NF + i] = NF + i - 1 if i == W else NF + i
    shift[ID_EX] = ID_EX; shift[ID_TD] = ID_TD
    x0 = {}
    for ids, sizes, _, _ in factors:
        for i in ids:
            x0.setdefault(i, np.array(blk(i), dtype=np.float64).copy())
    return factors, dropped, shift, x0


def _to_int(a, e_common):
    """doubles -> python integers, a = int * 2^e_common exactly"""
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for k, x in enumerate(np.asarray(a, dtype=np.float64).reshape(-1)):
        if x == 0.0:
            flat[k] = 0
        else:
            m, e = math.frexp(float(x))
            flat[k] = int(m * 9007199254740992.0) << (e - 53 - e_common)
    return out


def exact_prior_products(opts, win, prior, state, perturb_seed=None, near_cut=None):
    """The exact new prior of `win` linearised at `state`. Returns a dict: Lam [n, n], b [n] (doubles rounded from the 60-digit values), r0sq = b^T Lam^+ b, blocks (the kept
    block table: shifted id, size, idx, x0), m, n, rank, keep (n x rank orthonormal basis of the retained subspace, None when nothing is cut), eig_mm / eig_kept (extreme
    eigenvalues, for the records). None when the reference leaves the prior unchanged. perturb_seed: every row entry times 1 + delta, |delta| <= 2^-52.
    near_cut = (lo, hi): the case was built with ONE kept eigenvalue next to the cut on purpose; the exact eigenvalue must lie in [lo, hi], a side of 1e-8 known beforehand."""
    fr = factor_rows(opts, win, prior, state)
    if fr is None:
        return None
    factors, dropped, shift, x0 = fr
    loc = lambda s: 6 if s == 7 else s
    size_of = {}
    for ids, sizes, _, _ in factors:
        for i, s in zip(ids, sizes):
            size_of[i] = s
    order = sorted(dropped) + sorted(i for i in size_of if i not in dropped)
    off = {}; pos = 0
    for i in order:
        off[i] = pos; pos += loc(size_of[i])
    m = sum(loc(size_of[i]) for i in dropped); n = pos - m
    # sparse rows: (columns, values, residual)
    rows = []
    for ids, sizes, r, J in factors:
        cols = np.concatenate([off[i] + np.arange(loc(s)) for i, s in zip(ids, sizes)])
        vals = np.concatenate([Jb[:, :loc(s)] for Jb, s in zip(J, sizes)], axis=1)
        for k in range(len(r)):
            nz = np.nonzero(vals[k])[0]
            rows.append((cols[nz], vals[k, nz], r[k]))
    allv = np.concatenate([np.abs(v) for _, v, _ in rows] + [np.abs(np.array([r for _, _, r in rows]))])
    e_common = math.frexp(float(allv[allv > 0].min()))[1] - 53
    PB = 60                                                              # 1 + delta = (2^60 + d) / 2^60, |d| <= 2^8
    rng = np.random.default_rng(perturb_seed) if perturb_seed is not None else None
    A = np.zeros((pos, pos), dtype=object); b = np.zeros(pos, dtype=object)
    for cols, vals, r in rows:
        v = _to_int(vals, e_common); ri = _to_int(np.array([r]), e_common)[0]
        if rng is not None:
            d = rng.integers(-256, 257, size=len(v) + 1)
            v = np.array([int(x) * ((1 << PB) + int(dd)) for x, dd in zip(v, d[:-1])], dtype=object); ri = int(ri) * ((1 << PB) + int(d[-1]))
        A[np.ix_(cols, cols)] += np.outer(v, v); b[cols] += v * ri
    sh = 2 * e_common - (2 * PB if rng is not None else 0)
    with mp.workdps(DPS):
        to_mp = np.frompyfunc(lambda x: mp.ldexp(mp.mpf(x), sh), 1, 1)
        A = to_mp(A); b = to_mp(b)
        Af = np.array(A, dtype=np.float64)
        # ---- Amm: exactly zero rows are left out (the pseudo-inverse of a zero block); the rest must be regular far above the cut ---------------------------
        live = [k for k in range(m) if any(A[k, j] != 0 for j in range(m))]
        wmm = np.linalg.eigvalsh(Af[np.ix_(live, live)]) if live else np.array([np.inf])
        slack = 1e3 * np.finfo(float).eps * max(abs(wmm).max(), 1.0) if live else 0.0      # what eigvalsh can be wrong by
        if live and not wmm.min() - slack > BAND[1]:
            raise BadCase(f"Amm eigenvalues {wmm.min():.3e} .. {wmm.max():.3e}: not clear of the 1e-8 cut")
        n_dense = sum(loc(size_of[i]) for i in dropped if i < 2 * win.n_frames + 2)
        for k in [k for k in live if k >= n_dense] + [k for k in live if k < n_dense]:      # the features first, through the arrow: no fill-in among them
            nzc = np.array([j for j in range(pos) if j != k and (j >= m or j < n_dense and (k >= n_dense or j > k)) and (A[k, j] if j > k else A[j, k]) != 0], dtype=int)
            if len(nzc):
                row = np.array([A[k, j] if j > k else A[j, k] for j in nzc], dtype=object); col = row / A[k, k]
                for a, i in enumerate(nzc):                              # the upper triangle only: the matrix stays symmetric (nzc ascends)
                    A[i, nzc[a:]] -= col[a] * row[a:]
                b[nzc] -= col * b[k]
        K = np.triu(A[m:, m:]); K = K + np.triu(K, 1).T; bk = b[m:].copy()
        Kf = np.array(K, dtype=np.float64); Kf = 0.5 * (Kf + Kf.T)
        wk = np.linalg.eigvalsh(Kf)
        slack = 1e3 * np.finfo(float).eps * abs(wk).max()
        keep = None
        if wk.min() - slack > BAND[1]:                                   # nothing near the cut: Lam = K, r0sq by continuing the elimination
            eig_kept = (float(wk.min()), float(wk.max())); rank = n
            T = K.copy(); t = bk.copy(); r0sq = mp.mpf(0)
            for k in range(n):
                r0sq += t[k] * t[k] / T[k, k]
                row = T[k, k + 1:]; col = row / T[k, k]
                for a in range(n - k - 1):
                    T[k + 1 + a, k + 1 + a:] -= col[a] * row[a:]
                t[k + 1:] -= col * t[k]
            Lam, bb = K, bk
        else:                                                            # exact eigenvalues decide
            E, Q = mp.eigsy(mp.matrix(K.tolist()))
            ev = [E[i] for i in range(n)]
            inband = [float(e) for e in ev if BAND[0] <= e <= BAND[1]]
            if (inband and near_cut is None) or (near_cut is not None and not (len(inband) == 1 and near_cut[0] <= inband[0] <= near_cut[1] and not near_cut[0] <= EPS_CUT <= near_cut[1])):
                raise BadCase(f"kept-block eigenvalues in [1e-9, 1e-7]: {inband} (expected: {near_cut})")
            ret = [i for i in range(n) if ev[i] > EPS_CUT]
            eig_kept = (float(min(ev)), float(max(ev))); rank = len(ret)
            Lam = np.zeros((n, n), dtype=object); bb = np.zeros(n, dtype=object); r0sq = mp.mpf(0)
            for i in ret:
                v = np.array([Q[r, i] for r in range(n)], dtype=object)
                c = sum(v * bk)
                Lam = Lam + ev[i] * np.outer(v, v); bb = bb + c * v; r0sq += c * c / ev[i]
            if rank < n:
                keep = np.linalg.qr(np.array([[float(Q[r, i]) for i in ret] for r in range(n)]))[0]
        out = dict(Lam=np.array(Lam, dtype=np.float64), b=np.array(bb, dtype=np.float64), r0sq=float(r0sq), m=m, n=n, rank=rank, keep=keep,
                   eig_mm=(float(wmm.min()), float(wmm.max())), eig_kept=eig_kept)
    out["blocks"] = [dict(id=shift[i], size=size_of[i], idx=off[i] - m, x0=x0[i]) for i in order if i not in dropped]
    return out


def measures(Lam, b, r0sq, ref):
    """(e_Lambda, e_b, e_r) of a prior's products against the reference: entrywise errors scaled by sqrt(Lam_ii Lam_jj) and sqrt(Lam_ii) |r0|, both bounded by 1 for
    any J0, r0 (|b_i| <= sqrt(Lam_ii) |r0|), and the relative error of |r0|^2. Where the reference cuts directions, both sides are projected on its retained subspace."""
    Lr, br = ref["Lam"], ref["b"]
    if ref["keep"] is not None:
        P = ref["keep"] @ ref["keep"].T
        Lam = P @ Lam @ P; b = P @ b
    d = np.sqrt(np.diag(Lr))
    ok = np.diag(Lr) > 1e-40 * np.diag(Lr).max()                          # a coordinate that lies in the cut subspace altogether: zero up to the 60 digits
    r0n = math.sqrt(ref["r0sq"])
    eL = float(np.abs((Lam - Lr)[np.ix_(ok, ok)] / np.outer(d[ok], d[ok])).max())
    eb = float((np.abs(b - br)[ok] / d[ok]).max() / r0n)
    er = abs(r0sq - ref["r0sq"]) / ref["r0sq"]
    return eL, eb, er


def prior_measures(p, ref):
    J0, r0, _ = abi.prior_to_numpy(p)
    return measures(J0.T @ J0, J0.T @ r0, float(r0 @ r0), ref)


def bound(opts, win, prior, state, ref, oracle_prior, seed=1, near_cut=None):
    """The tolerance of one case, per measure: 10 x max(error of the fp64 oracle marginalized at the same state, change of the exact reference when every row entry
    moves by one rounding). Returns (tolerances, e_oracle, e_pert), three numbers each."""
    e_or = prior_measures(oracle_prior, ref)
    pert = exact_prior_products(opts, win, prior, state, perturb_seed=seed, near_cut=near_cut)
    e_pe = measures(pert["Lam"], pert["b"], pert["r0sq"], ref)
    return tuple(10.0 * max(a, c) for a, c in zip(e_or, e_pe)), e_or, e_pe
