"""The case list of the feature triangulation (include/vilfusion.h, "Feature manager: triangulate"), shared by the CPU and the GPU tests of
test_feature_triangulate.py. A case is one call: a name and a list of tables (FeatureManager.triangulation_table's dict). Everything is seeded; nothing here
depends on the library. The references of all cases are computed once (references()) and shared."""
import functools
import numpy as np
import tri_reference as ref

WINDOW_SIZE = 10
NF = WINDOW_SIZE + 1
INIT_DEPTH = 5.0
FOCAL = 460.0
# config/kitti/kitti_config.yaml:10-23, the rotation made orthonormal (its six digits are not): a true depth is then the depth of the text to rounding
_U, _, _VT = np.linalg.svd(np.array([[0.00781297, -0.0042792, 0.99996], [-0.999859, -0.014868, 0.00774856], [0.0148343, -0.99988, -0.00439476]]))
RIC = _U @ _VT
TIC = np.array([1.1439, -0.312718, 0.726546])
NAN = float("nan")


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def poses(seed, n_frames=NF, step=0.5, one_pose=False, offset=None):
    """body poses of a drive with `step` metres between frames, mostly sideways to the camera so that close points keep parallax; one_pose: every frame the same"""
    rng = np.random.default_rng(seed)
    R0 = rot(rng.normal(size=3), rng.uniform(0, np.pi))
    P0 = rng.uniform(-20, 20, 3) if offset is None else np.asarray(offset, dtype=np.float64)
    d = R0 @ (np.array([0.5, 0.85, 0.1]) / np.linalg.norm([0.5, 0.85, 0.1]))
    Ps, Rs = [], []
    for k in range(n_frames):
        kk = 0 if one_pose else k
        Ps.append(P0 + kk * step * d + (0 if one_pose else rng.normal(0, 0.02 * step, 3)))
        Rs.append(R0 @ rot([0.2, 0.1, 1.0], 0.01 * kk))
    return np.array(Ps), np.array(Rs)


def observe(rng, Ps, Rs, tic, ric, start, n_obs, true_depth, noise_px=0.0, scale=1.0):
    """the observations of a point at true_depth along a random ray of the camera of frame `start` (a negative depth: behind the camera); scale: z of the points"""
    Rc = Rs @ ric
    tc = Ps + Rs @ tic
    ray = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), 1.0])
    X = Rc[start] @ (true_depth * ray) + tc[start]
    out = []
    for j in range(start, start + n_obs):
        pc = Rc[j].T @ (X - tc[j])
        p = np.array([pc[0] / pc[2] + rng.normal(0, noise_px / FOCAL) if noise_px else pc[0] / pc[2], pc[1] / pc[2] + rng.normal(0, noise_px / FOCAL) if noise_px else pc[1] / pc[2], 1.0])
        out.append(scale * p)
    return out


class Builder:
    def __init__(self, seed, n_frames=NF, step=0.5, one_pose=False, noise_px=0.0, tic=TIC, ric=RIC, offset=None):
        self.rng = np.random.default_rng(seed + 99)
        self.Ps, self.Rs = poses(seed, n_frames, step, one_pose, offset)
        self.tic, self.ric, self.noise = np.array(tic, dtype=np.float64), np.array(ric, dtype=np.float64), noise_px
        self.start, self.first, self.pts, self.depth, self.truth = [], [0], [], [], []

    def add(self, n_obs, start=0, depth_in=-1.0, true_depth=None, scale=1.0, points=None):
        td = float(self.rng.uniform(4.0, 30.0)) if true_depth is None else true_depth
        obs = observe(self.rng, self.Ps, self.Rs, self.tic, self.ric, start, n_obs, td, self.noise, scale) if points is None else [np.array(p, dtype=np.float64) for p in points]
        self.start.append(start); self.pts.extend(obs); self.first.append(len(self.pts)); self.depth.append(depth_in); self.truth.append(td)
        return self

    def table(self):
        return dict(n_frames=len(self.Ps), Ps=self.Ps.copy(), Rs=self.Rs.copy(), tic=self.tic, ric=self.ric, start_frame=np.array(self.start, dtype=np.int32),
                    first_obs=np.array(self.first, dtype=np.int32), points=np.array(self.pts, dtype=np.float64).reshape(-1, 3),
                    depth=np.array(self.depth, dtype=np.float64), truth=np.array(self.truth, dtype=np.float64))


def edge_window(seed, step, noise_px):
    """every per-feature case of one step size: track lengths 1 / 2 / 3 / 11, start frames 0 / WINDOW_SIZE - 3 / WINDOW_SIZE - 2, depth_in 7.5 / 0 / -1 / NaN,
    a point behind the camera, a point whose z is not 1; at 5 mm steps and without noise the two depths on either side of the reset threshold"""
    one = step == 0.0
    b = Builder(seed, NF, step if not one else 0.5, one_pose=one, noise_px=noise_px)
    near = 8.0 if step >= 0.1 else 0.12                     # 5 mm steps: points close enough to have parallax
    for n_obs in (1, 2, 3, 11):
        for din in (7.5, 0.0, -1.0, NAN):
            b.add(n_obs, 0, din, true_depth=near * (1 + 0.1 * n_obs))
    for start, lens in ((WINDOW_SIZE - 3, (2, 4)), (WINDOW_SIZE - 2, (2, 3))):
        for n_obs in lens:
            for din in (7.5, -1.0):
                b.add(n_obs, start, din, true_depth=near)
    b.add(3, 2, -1.0, true_depth=-near)                      # behind the camera: reset
    b.add(5, 1, 0.0, true_depth=near, scale=2.5)             # z = 2.5
    b.add(4, 3, -1.0, true_depth=near, scale=-1.5)           # z = -1.5: the ray points backwards, the constraint is the same
    if step == 0.005 and noise_px == 0.0:
        b.add(3, 0, -1.0, true_depth=0.0999)
        b.add(3, 0, -1.0, true_depth=0.1001)
        b.add(6, 2, 0.0, true_depth=0.0999)
        b.add(6, 2, 0.0, true_depth=0.1001)
    return b.table()


def count_window(seed, n_features, n_candidates, n_frames=NF, short=True):
    """n_features features of which exactly n_candidates are candidates (spread over the list); the others have a depth or are not used"""
    b = Builder(seed, n_frames, 0.5, noise_px=0.5)
    pick = set(np.round(np.linspace(0, n_features - 1, n_candidates)).astype(int).tolist()) if n_candidates else set()
    assert len(pick) == n_candidates
    last = min(WINDOW_SIZE - 3, n_frames - 2)
    for f in range(n_features):
        start = int(b.rng.integers(0, last + 1))
        n_obs = int(b.rng.integers(2, min(4 if short else NF, n_frames - start) + 1))
        if f in pick:
            b.add(n_obs, start, [-1.0, 0.0, NAN][f % 3])
        elif f % 4 == 3:
            b.add(1, int(b.rng.integers(0, n_frames)), -1.0)             # one observation: not used
        else:
            b.add(n_obs, start, float(b.rng.uniform(3.0, 40.0)))
    return b.table()


def special_window():
    """points that are not finite or zero (not screened: NaN, kept and flagged), and positions 1e160 apart (the last column's norm overflows, its pairs are skipped,
    the winner has V_3 = 0 exactly: +-inf)"""
    b = Builder(7, NF, 0.5)
    b.add(2, 0, -1.0, points=[[0.1, 0.2, 1.0], [NAN, 0.2, 1.0]])
    b.add(3, 1, -1.0, points=[[0.1, 0.2, 1.0], [float("inf"), 0.2, 1.0], [0.1, 0.1, 1.0]])
    b.add(2, 4, 0.0, points=[[0.0, 0.0, 0.0], [0.1, 0.2, 1.0]])
    b.add(4, 0, -1.0)
    t1 = b.table()
    h = Builder(8, NF, 0.5)
    h.Ps = h.Ps * 1e160
    for k in range(6):
        h.add(2 + k % 3, k, -1.0, points=[[0.05 * (k - 2), -0.04 * k, 1.0]] * (2 + k % 3))
    return [t1, h.table()]


@functools.lru_cache(maxsize=None)
def cases():
    """-> list of (name, [tables])"""
    out = []
    for step in (0.5, 0.005, 0.0):
        for noise in (0.0, 0.5):
            out.append((f"edges step {step} noise {noise}", [edge_window(100 + int(step * 1000) + int(noise * 10), step, noise)]))
    b2 = Builder(21, 2, 0.5, noise_px=0.5)
    for din in (-1.0, 7.5, 0.0, NAN):
        b2.add(2, 0, din)
    b2.add(1, 1, -1.0)
    out.append(("two frames", [b2.table()]))
    out.append(("no features", [Builder(22).table()]))
    out.append(("one feature", [Builder(23, noise_px=0.5).add(3, 2, -1.0).table()]))
    out.append(("1000 features", [count_window(24, 1000, 100)]))
    for n in (0, 1, 63, 64, 65):
        out.append((f"{n} candidates", [count_window(30 + n, 80, n)]))
    # one window's candidates straddle the boundary of a workgroup of 64, candidate-free windows between windows that have some
    out.append(("straddle", [count_window(40, 50, 40), count_window(41, 20, 0), Builder(42).table(), count_window(43, 60, 40), count_window(44, 5, 0), count_window(45, 12, 10)]))
    out.append(("two windows", [count_window(50, 9, 3, short=False), count_window(51, 7, 2, n_frames=5)]))
    out.append(("three windows", [count_window(52, 6, 2), count_window(53, 1, 1), count_window(54, 4, 0)]))
    out.append(("300 windows", [count_window(1000 + w, 3, 1 + (w % 7 == 0)) for w in range(300)]))
    out.append(("special", special_window()))
    return out


@functools.lru_cache(maxsize=None)
def references():
    """the restatement's result of every table of every case, computed once and shared: {name: [result per table]}"""
    return {name: [ref.triangulate(t, WINDOW_SIZE, INIT_DEPTH) for t in tables] for name, tables in cases()}


def random_features(seed, n):
    """n seeded random candidates, one per table of their own: 2 to 11 observations, start frames 0 to 7, steps of 0.5 m / 5 mm / 0, close points, points behind the
    camera, depth_in -1 / 0 / NaN / 7.5 -> list of tables"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        step = [0.5, 0.005, 0.0][int(rng.integers(0, 3))]
        start = int(rng.integers(0, WINDOW_SIZE - 2))
        n_obs = int(rng.integers(2, NF - start + 1))
        b = Builder(seed * 1000 + k, NF, step if step else 0.5, one_pose=step == 0.0, noise_px=[0.0, 0.5][int(rng.integers(0, 2))])
        td = float(rng.uniform(0.05, 0.15)) if rng.uniform() < 0.3 else float(rng.uniform(2.0, 40.0))
        if rng.uniform() < 0.15:
            td = -td
        b.add(n_obs, start, [-1.0, 0.0, NAN, 7.5][int(rng.integers(0, 4))], true_depth=td)
        out.append(b.table())
    return out
