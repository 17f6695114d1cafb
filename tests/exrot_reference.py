"""numpy restatement of the camera-IMU rotation calibration, written from the contract text in include/vilfusion.h ("Camera-IMU rotation calibration").

Every float operation is one numpy operation on float64 values (the points are rounded to float32 first, as the text says), so it is rounded on its own; sums are
written out in the text's order. The search is frontend_reference's and the decomposition and the depths are startup_reference's, imported and not copied. No code
is shared with csrc."""
import numpy as np
from frontend_reference import hypotheses, inliers, jacobi, MAX_HYPOTHESES
from startup_reference import decompose, depths

COUNT, HYPOTHESIS, FINITE, SOLVED, SKIPPED = 1, 2, 4, 7, 8
MAX_SLOTS, MAX_HISTORY = 256, 256
DEFAULTS = dict(n_hypotheses=512, seed=0, min_corres=9, min_frames=10, ransac_threshold=3.0, huber_deg=5.0, min_sigma=0.25)
DEG = np.float64(57.29577951308232)
HALF_PI = np.float64(1.5707963267948966)
F = np.float64


def q_to_R(q):
    """Q = R(q) of the PnP's paragraph "candidate" with (x, y, z, s) = q, not normalised"""
    x, y, z, s = (F(v) for v in q)
    with np.errstate(all="ignore"):
        return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - s * z), 2.0 * (x * z + s * y)],
                         [2.0 * (x * y + s * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - s * x)],
                         [2.0 * (x * z - s * y), 2.0 * (y * z + s * x), 1.0 - 2.0 * (x * x + y * y)]], dtype=np.float64)


def quat(M):
    """Eigen's matrix-to-quaternion -> (x, y, z, w)"""
    M = np.asarray(M, dtype=np.float64)
    q = np.zeros(4)
    with np.errstate(all="ignore"):
        tr = (M[0, 0] + M[1, 1]) + M[2, 2]
        if tr > 0.0:
            s = np.sqrt(tr + 1.0)
            q[3] = 0.5 * s
            u = 0.5 / s
            q[0], q[1], q[2] = (M[2, 1] - M[1, 2]) * u, (M[0, 2] - M[2, 0]) * u, (M[1, 0] - M[0, 1]) * u
        else:
            i = 0
            if M[1, 1] > M[0, 0]:
                i = 1
            if M[2, 2] > M[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            s = np.sqrt(((M[i, i] - M[j, j]) - M[k, k]) + 1.0)
            q[i] = 0.5 * s
            u = 0.5 / s
            q[3] = (M[k, j] - M[j, k]) * u
            q[j] = (M[j, i] + M[i, j]) * u
            q[k] = (M[k, i] + M[i, k]) * u
    return q


def atan2p(y, x):
    """the arc tangent of y / x for y, x >= 0 in + - * / sqrt"""
    y, x = F(y), F(x)
    with np.errstate(all="ignore"):
        swapped = bool(y > x)
        lo, hi = (x, y) if swapped else (y, x)
        q = F(0.0) if hi == 0.0 else lo / hi
        for _ in range(3):
            q = q / (1.0 + np.sqrt(1.0 + q * q))
        z = q * q
        s = F(1.0) / F(15.0)
        for n in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            s = F(1.0) / F(n) - z * s
        s = 1.0 - z * s
        r = (q * s) * 8.0
        return HALF_PI - r if swapped else r


def angle_deg(Rc, Rcg):
    x1, y1, z1, w1 = quat(Rc)
    x2, y2, z2, w2 = quat(Rcg)
    xc, yc, zc, wc = -x2, -y2, -z2, w2
    with np.errstate(all="ignore"):
        dw = ((w1 * wc - x1 * xc) - y1 * yc) - z1 * zc
        dx = ((w1 * xc + x1 * wc) + y1 * zc) - z1 * yc
        dy = ((w1 * yc + y1 * wc) + z1 * xc) - x1 * zc
        dz = ((w1 * zc + z1 * wc) + x1 * yc) - y1 * xc
        return DEG * (2.0 * atan2p(np.sqrt((dx * dx + dy * dy) + dz * dz), np.abs(dw)))


def block(Rc, Rimu, weight):
    """B = weight (L - R) [4][4]"""
    x, y, z, w = quat(Rc)
    L = np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])
    x, y, z, w = quat(Rimu)
    R = np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])
    with np.errstate(all="ignore"):
        return F(weight) * (L - R)


def mat3(A, B):
    """C_rc = (A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c"""
    C = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
    return C


def solve_relative_r(a, b, frame_count, P):
    """solveRelativeR -> dict(flags, count, best_k, score, front, chosen, Rc)"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 2).astype(np.float32), np.asarray(b, dtype=np.float64).reshape(-1, 2).astype(np.float32)
    m = len(a)
    row = dict(flags=0, count=m, best_k=-1, score=0, front=[0, 0, 0, 0], chosen=-1, Rc=np.eye(3))
    if m < P["min_corres"] or m < 8:
        return row
    row["flags"] |= COUNT
    K = int(P["n_hypotheses"])
    assert 1 <= K <= MAX_HYPOTHESES
    Fs, valid = hypotheses(a, b, K, (int(P["seed"]) + frame_count) & 0xffffffff)
    inl = inliers(Fs, a, b, P["ransac_threshold"])
    score = np.where(valid, inl.sum(axis=1), -1)
    k = int(np.argmax(score))
    if score[k] < 0:
        return row
    row.update(flags=row["flags"] | HYPOTHESIS, best_k=k, score=int(score[k]))
    R1, R2, t = decompose(Fs[k])
    if not (np.isfinite(R1).all() and np.isfinite(R2).all() and np.isfinite(t).all()):
        return row
    front = []
    with np.errstate(all="ignore"):
        for R in (R1, R2):
            z1, z2 = depths(R, t, a, b)
            front += [int(((z1 > 0.0) & (z2 > 0.0)).sum()), int(((-z1 > 0.0) & (-z2 > 0.0)).sum())]
    chosen = 0 if max(front[0], front[1]) > max(front[2], front[3]) else 1
    row.update(flags=row["flags"] | FINITE, front=front, chosen=chosen, Rc=(R1 if chosen == 0 else R2).T.copy())
    return row


class Calibrator:
    """one slot"""

    def __init__(self, keep=False, **params):
        self.P = dict(DEFAULTS, **params)
        self.keep = keep
        self.reset()

    def reset(self):
        self._kept = []
        self.frame_count = 0
        self.ric = np.eye(3)
        self.Rc, self.Rimu, self.Rcg = [], [], []
        self.angles, self.weights = np.zeros(0), np.zeros(0)

    def entry(self, i):
        """(angle, weight, B) of history entry i (0-based)"""
        hub = F(self.P["huber_deg"])
        ang = angle_deg(self.Rc[i], self.Rcg[i])
        with np.errstate(all="ignore"):
            wgt = hub / ang if ang > hub else F(1.0)
        return ang, wgt, block(self.Rc[i], self.Rimu[i], wgt)

    def system(self):
        """the weights of every entry and G [4][4] (before the Jacobi), with the blocks B [n][4][4]. Every entry is computed anew on every push, as the text says;
        keep=True (the constructor) keeps the entries of earlier pushes instead, which gives the same numbers (an entry's inputs never change) in less time"""
        n = self.frame_count
        if self.keep:
            self._kept += [self.entry(i) for i in range(len(self._kept), n)]
            ent = self._kept
        else:
            ent = [self.entry(i) for i in range(n)]
        ang, wgt = np.array([e[0] for e in ent]), np.array([e[1] for e in ent])
        B = np.array([e[2] for e in ent]).reshape(n, 4, 4)
        G = np.zeros((4, 4))
        with np.errstate(all="ignore"):
            for p in range(4):
                for q in range(p, 4):
                    terms = (B[:, :, p] * B[:, :, q]).reshape(-1)                 # i ascending, within i the rows r = 0 .. 3
                    G[p, q] = G[q, p] = np.cumsum(np.concatenate([[0.0], terms]))[-1]      # np.cumsum adds one term at a time in index order, from 0.0
        return ang, wgt, B, G

    def push(self, a, b, delta_q):
        if self.frame_count >= MAX_HISTORY:
            raise ValueError("the slot is full")
        P = self.P
        row = solve_relative_r(a, b, self.frame_count, P)
        Rimu = q_to_R(delta_q)
        Rcg = mat3(mat3(self.ric.T, Rimu), self.ric)
        self.frame_count += 1
        self.Rc.append(row["Rc"]); self.Rimu.append(Rimu); self.Rcg.append(Rcg)
        ang, wgt, _, G = self.system()
        self.angles, self.weights = ang, wgt
        G = G.reshape(1, 4, 4).copy()
        with np.errstate(all="ignore"):
            V = jacobi(G, 4)[0]
            g = np.array([G[0, k, k] for k in range(4)])
            sig = np.array([np.sqrt(v) if v > 0.0 else F(0.0) for v in g])
        at = 0
        for k in range(1, 4):
            if g[k] < g[at]:
                at = k
        x = V[:, at].copy()
        sigma = np.sort(sig)[::-1].copy()
        self.ric = q_to_R(x).T.copy()
        ok = bool(self.frame_count >= P["min_frames"] and sigma[2] > P["min_sigma"])
        row.update(frame_count=self.frame_count, ok=ok, angle=ang[-1], weight=wgt[-1], sigma=sigma, x=x, ric=self.ric.copy())
        return row

    def skipped(self):
        """the row of a slot whose pair had n = -1"""
        return dict(frame_count=self.frame_count, flags=SKIPPED, count=-1, best_k=-1, score=0, front=[0, 0, 0, 0], chosen=-1, ok=False, Rc=np.zeros((3, 3)),
                    angle=F(0.0), weight=F(0.0), sigma=np.zeros(4), x=np.zeros(4), ric=self.ric.copy())

    def history(self):
        n = self.frame_count
        return dict(count=n, Rc=np.array(self.Rc).reshape(n, 3, 3), Rimu=np.array(self.Rimu).reshape(n, 3, 3), Rcg=np.array(self.Rcg).reshape(n, 3, 3),
                    angle=self.angles.copy(), weight=self.weights.copy())


class Backend:
    """a pure-Python back-end surface for SlidingWindowEstimator: ex_rotation(pairs) is the restatement, one slot"""

    def __init__(self, **params):
        self.cal = Calibrator(**params)

    def ex_rotation(self, pairs):
        (a, b, dq), = pairs
        return [self.cal.push(a, b, dq)]
