"""numpy restatement of the second stage of the visual loop closure, PnP-RANSAC and the loop decision, written from the contract text in include/vilfusion.h
("Visual loop closure, second stage").

Every float operation is one numpy elementwise operation on float64 values, so it is rounded on its own; sums are written out in the text's order. The residual, the
LDL^T, the candidate and the whole refit (solveFrameByPnP) are sfm_reference's, the match is kf_reference's and the draw is frontend_reference's: imported, not
copied. The hypotheses run side by side as a trailing array axis through those same functions. No code is shared with csrc. KeyFrameStore has the shape of
vil_fusion_amd.estimator.KeyFrameStore, so a test drives both with the same calls."""
import numpy as np
import sfm_reference as sr
import kf_reference as kr
import frontend_reference as fr

GATE, NO_HYPOTHESIS, REFIT, REFIT_DROPPED, LOOP = 1, 2, 4, 8, 16
SLOTS = 5
DEFAULTS = dict(n_hypotheses=256, seed=0, hyp_iterations=5, refine_iterations=10, min_loop_num=25, lambda0=1e-3, reproj_threshold=10.0 / 460.0, max_yaw=30.0, max_dist=20.0)
ROW_KEYS = ("n_matched", "n_inliers", "best_k", "flags", "has_loop", "accepted", "R", "t", "PnP_R_old", "PnP_T_old", "relative_t", "relative_q", "relative_yaw", "cost0", "cost1")


def samples(m, K, seed):
    """int64 [K][5]: the paragraph "sample" with 5 slots and n = m"""
    assert m >= SLOTS
    k = np.arange(K, dtype=np.uint64)
    S = np.zeros((K, SLOTS), dtype=np.int64)
    for j in range(SLOTS):
        idx = ((fr.draw(seed, k, j) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
        for _ in range(j):
            dup = (idx[:, None] == S[:, :j]).any(axis=1)
            idx = np.where(dup, (idx + 1) % m, idx)
        S[:, j] = idx
    return S


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def guess(vio_R, vio_T, qic, tic):
    """-> (R0, t0) of the paragraph "guess" """
    R, T, q, c = (np.asarray(a, dtype=np.float64) for a in (vio_R, vio_T, qic, tic))
    Rwc = np.array([[dot3(R[r, 0], q[0, k], R[r, 1], q[1, k], R[r, 2], q[2, k]) for k in range(3)] for r in range(3)])
    Twc = np.array([T[r] + dot3(R[r, 0], c[0], R[r, 1], c[1], R[r, 2], c[2]) for r in range(3)])
    R0 = Rwc.T.copy()
    return R0, np.array([-dot3(R0[r, 0], Twc[0], R0[r, 1], Twc[1], R0[r, 2], Twc[2]) for r in range(3)])


def ordered_sum(terms):
    """terms [j][...] -> the sum over j from 0.0 in order"""
    s = np.zeros(terms[0].shape)
    for v in terms:
        s = s + v
    return s


def hypotheses(X, u, S, R0, t0, iterations, lambda0):
    """the K hypotheses side by side: X [m][3], u [m][2] (float64 values of float32), S [K][5] -> (R [3][3][K], t [3][K])"""
    K = len(S)
    Xs, us = np.transpose(X[S], (1, 2, 0)), np.transpose(u[S], (1, 2, 0))        # [5][3][K], [5][2][K]: sr.residuals reads X[:, c] and u[:, c]
    R, t = np.repeat(np.asarray(R0, dtype=np.float64)[:, :, None], K, axis=2), np.repeat(np.asarray(t0, dtype=np.float64)[:, None], K, axis=1)
    lam = np.full(K, np.float64(lambda0))
    zero = np.zeros((SLOTS, K))
    with np.errstate(all="ignore"):
        for _ in range(int(iterations)):
            q, iz, xn, yn, e0, e1 = sr.residuals(R, t, Xs, us)
            c0, c1 = xn * iz, yn * iz
            J0 = [-(c0 * q[1]), iz * q[2] + c0 * q[0], -(iz * q[1]), iz, zero, -c0]
            J1 = [-(iz * q[2] + c1 * q[1]), c1 * q[0], iz * q[0], zero, iz, -c1]
            s = [ordered_sum(J0[a] * J0[b] + J1[a] * J1[b]) for a, b in sr.UPPER] + [ordered_sum(J0[a] * e0 + J1[a] * e1) for a in range(6)] + [ordered_sum(e0 * e0 + e1 * e1)]
            cost = s[27]
            x6, pos = np.zeros((6, K)), np.zeros(K, dtype=bool)
            for k in range(K):
                Hd = np.zeros((6, 6))
                for i, (a, b) in enumerate(sr.UPPER):
                    Hd[a, b] = s[i][k] + lam[k] * s[i][k] if a == b else s[i][k]
                x = sr.ldlt_solve(Hd, -np.array([s[21 + a][k] for a in range(6)]))
                if x is not None:
                    x6[:, k], pos[k] = x, True
            Rn, tn = sr.candidate(R, t, x6)
            _, _, _, _, f0, f1 = sr.residuals(Rn, tn, Xs, us)
            cn = ordered_sum(f0 * f0 + f1 * f1)
            ok = pos & (cn < cost)
            R, t = np.where(ok, Rn, R), np.where(ok, tn, t)
            lam = np.where(ok, lam / np.float64(10.0), lam * np.float64(10.0))
    return R, t


def inliers(R, t, X, u, thr2):
    """the paragraph "score" for poses R [3][3][...], t [3][...] against every member -> bool [...][m]"""
    with np.errstate(all="ignore"):
        q, _, _, _, e0, e1 = sr.residuals(R[..., None], t[..., None], X, u)
        return ((q[2] + t[2][..., None]) > 0) & ((e0 * e0 + e1 * e1) <= thr2)


def pose_out(R, t, qic, tic):
    q, c = np.asarray(qic, dtype=np.float64), np.asarray(tic, dtype=np.float64)
    W = R.T.copy()
    Tw = np.array([-dot3(R[0, r], t[0], R[1, r], t[1], R[2, r], t[2]) for r in range(3)])
    P = np.array([[dot3(W[r, 0], q[k, 0], W[r, 1], q[k, 1], W[r, 2], q[k, 2]) for k in range(3)] for r in range(3)])
    return P, np.array([Tw[r] - dot3(P[r, 0], c[0], P[r, 1], c[1], P[r, 2], c[2]) for r in range(3)])


def yaw_deg(R):
    return np.arctan2(R[1, 0], R[0, 0]) / np.pi * 180.0


def normalize_angle(a):
    a = np.float64(a)
    return a - 360.0 * np.floor((a + 180.0) / 360.0) if a > 0 else a + 360.0 * np.floor((-a + 180.0) / 360.0)


def quaternion(M):
    """Eigen's matrix-to-quaternion rule -> (w, x, y, z)"""
    q = np.zeros(4)
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        q[0] = 0.5 * s
        s = 0.5 / s
        q[1], q[2], q[3] = (M[2, 1] - M[1, 2]) * s, (M[0, 2] - M[2, 0]) * s, (M[1, 0] - M[0, 1]) * s
    else:
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
        q[1 + i] = 0.5 * s
        s = 0.5 / s
        q[0], q[1 + j], q[1 + k] = (M[k, j] - M[j, k]) * s, (M[j, i] + M[i, j]) * s, (M[k, i] + M[i, k]) * s
    return q


def decide(P, PT, vio_R, vio_T, max_yaw=30.0, max_dist=20.0):
    """the paragraph "decision" -> (relative_t, relative_q, relative_yaw, has_loop)"""
    P, PT, Rv, Tv = (np.asarray(a, dtype=np.float64) for a in (P, PT, vio_R, vio_T))
    dT = Tv - PT
    rt = np.array([P[0, a] * dT[0] + P[1, a] * dT[1] + P[2, a] * dT[2] for a in range(3)])
    M = np.array([[P[0, a] * Rv[0, b] + P[1, a] * Rv[1, b] + P[2, a] * Rv[2, b] for b in range(3)] for a in range(3)])
    yaw = normalize_angle(yaw_deg(Rv) - yaw_deg(P))
    dist = np.sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2])
    return rt, quaternion(M), yaw, bool(abs(yaw) < max_yaw and dist < max_dist)


def empty_row(n_matched=0, flags=0):
    return dict(n_matched=int(n_matched), n_inliers=0, best_k=-1 if flags == NO_HYPOTHESIS else 0, flags=flags, has_loop=False, accepted=0, R=np.zeros((3, 3)), t=np.zeros(3),
                PnP_R_old=np.zeros((3, 3)), PnP_T_old=np.zeros(3), relative_t=np.zeros(3), relative_q=np.zeros(4), relative_yaw=np.float64(0.0), cost0=np.float64(0.0),
                cost1=np.float64(0.0))


def pnp_ransac(X, u, old_index, vio_R, vio_T, qic, tic, **params):
    """one old key frame: X [m][3], u [m][2] float32 in S order -> (row, mask over S bool [m])"""
    P = dict(DEFAULTS, **params)
    X, u = np.asarray(X, dtype=np.float32).reshape(-1, 3).astype(np.float64), np.asarray(u, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    m = len(X)
    if m <= P["min_loop_num"]:
        return empty_row(m, GATE), np.zeros(m, dtype=bool)
    R0, t0 = guess(vio_R, vio_T, qic, tic)
    K = int(P["n_hypotheses"])
    S = samples(m, K, (int(P["seed"]) + int(old_index)) & 0xffffffff)
    R, t = hypotheses(X, u, S, R0, t0, P["hyp_iterations"], P["lambda0"])
    thr2 = np.float64(P["reproj_threshold"]) * np.float64(P["reproj_threshold"])
    valid = np.isfinite(R).all(axis=(0, 1)) & np.isfinite(t).all(axis=0)
    score = np.where(valid, inliers(R, t, X, u, thr2).sum(axis=1), -1)
    best = int(np.argmax(score))                     # the first of the highest
    if score[best] < 0:
        return empty_row(m, NO_HYPOTHESIS), np.zeros(m, dtype=bool)
    Rw, tw = R[:, :, best].copy(), t[:, best].copy()
    mask = inliers(Rw, tw, X, u, thr2)
    fit = sr.pnp(X[mask], u[mask], Rw, tw, 0, warn_pnp_count=0, pnp_iterations=int(P["refine_iterations"]), lambda0=P["lambda0"])
    row = empty_row(m)
    kept = bool(fit["flags"] & sr.POSE)
    Rf, tf = (fit["R"], fit["t"]) if kept else (Rw, tw)
    row.update(n_inliers=int(mask.sum()), best_k=best, flags=REFIT if kept else REFIT_DROPPED, accepted=fit["accepted"], cost0=fit["cost0"], cost1=fit["cost1"], R=Rf.copy(), t=tf.copy())
    row["PnP_R_old"], row["PnP_T_old"] = pose_out(Rf, tf, qic, tic)
    if row["n_inliers"] > P["min_loop_num"]:
        row["relative_t"], row["relative_q"], row["relative_yaw"], row["has_loop"] = decide(row["PnP_R_old"], row["PnP_T_old"], vio_R, vio_T, P["max_yaw"], P["max_dist"])
        if row["has_loop"]:
            row["flags"] |= LOOP
    return row, mask


class KeyFrameStore(kr.KeyFrameStore):
    def set_geometry(self, index, point_3d, vio_R, vio_T):
        f = self.frames[index]
        X = np.array(point_3d, dtype=np.float32).reshape(-1, 3)
        assert len(X) == len(f["window_uv"])
        f["geometry"] = (X, np.array(vio_R, dtype=np.float64).reshape(3, 3), np.array(vio_T, dtype=np.float64).reshape(3))

    def findConnection(self, cur, olds, qic, tic, point_id=None, **params):
        X, vio_R, vio_T = self.frames[cur]["geometry"]
        res = self.searchByBRIEFDes(cur, olds)
        out = []
        for i, o in enumerate(olds):
            on = res["status"][i] != 0
            row, mask = pnp_ransac(X[on], res["pt_old_norm"][i][on], o, vio_R, vio_T, qic, tic, **params)
            status = np.zeros(len(X), dtype=np.uint8)
            status[np.flatnonzero(on)[mask]] = 1
            row["loop_info"] = np.concatenate([row["relative_t"], row["relative_q"], [row["relative_yaw"]]]) if row["has_loop"] else None
            row["status"] = status
            if point_id is not None:
                ids = np.asarray(point_id).reshape(len(X))
                row["match_points"] = np.concatenate([res["pt_old_norm"][i][status != 0], ids[status != 0].astype(np.float32).reshape(-1, 1)], axis=1).astype(np.float32).reshape(-1, 3)
            out.append(row)
        return out
