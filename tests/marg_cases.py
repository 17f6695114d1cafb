"""The windows of tests/test_marginalization.py: synthetic 11-frame windows shaped to sit on the edges of the marginalization kernels (vilf_marg.hip) — the dropped-feature
count against the 16-row chunks and the LDS limit of the Jacobi solver, the frame-0 factor count against the gather chunks and the slot table, both dropped dense sizes,
the kept dimensions, priors with a chosen spectrum next to the 1e-8 cut, gauge-deficient windows. CPU only: numpy and vil_fusion_amd.synth."""
import numpy as np
from vil_fusion_amd import abi, synth

NF = 11
TEMPER = 1e6          # factor on every vilf_imu_preint.covariance: Amm 4e2 .. 2.5e8 instead of 6.6e3 .. 2.5e14, fp64 resolves every block
_C0, _C1 = abi.IMU_OFF["covariance"]


def temper(win, scale=TEMPER):
    win.imu[:, _C0:_C1] *= scale
    return win


def frame0_counts(win):
    """(mf, f0): features that start in frame 0 and their projection factors"""
    s0 = win.feature_start_frame == 0
    return int(s0.sum()), int((np.diff(win.feature_obs_offset) - 1)[s0].sum())


def spread(mf, f0):
    """mf track lengths (factors per feature, 1 .. 10) that sum to f0, as even as possible"""
    if mf == 0:
        assert f0 == 0
        return []
    base, rem = divmod(f0, mf)
    assert 1 <= base and base + (1 if rem else 0) <= NF - 1, (mf, f0)
    return [base + 1] * rem + [base] * (mf - rem)


def shape_window(win, mf, f0=None, track_lengths=None, n_other=30):
    """A window with exactly `mf` features that start in frame 0 and `f0` projection factors of theirs, built from the features of `win`: the longest frame-0 tracks are
    selected (tracks that start later are re-anchored to frame 0 when there are too few) and trimmed from their end to `track_lengths` factors each (default: f0 spread
    evenly; f0 None: 1 + i % 5). `n_other` later-starting features stay as they are. Feature order, feature_const, the offsets, obs_point and the td inputs follow."""
    if track_lengths is None:
        track_lengths = spread(mf, f0) if f0 is not None else [1 + i % 5 for i in range(mf)]
    assert len(track_lengths) == mf and (f0 is None or sum(track_lengths) == f0)
    nfac = np.diff(win.feature_obs_offset) - 1
    start = win.feature_start_frame.copy()
    first = sorted(np.where(start == 0)[0], key=lambda k: -nfac[k])
    later = sorted(np.where(start != 0)[0], key=lambda k: -nfac[k])
    want = sorted(track_lengths, reverse=True)
    take = {}
    for L in want:
        if first and nfac[first[0]] >= L:
            take[first.pop(0)] = L
        else:                                       # re-anchor: the track's observations now count from frame 0
            assert later and nfac[later[0]] >= L, "not enough tracks of this length in the source window"
            k = later.pop(0); start[k] = 0; take[k] = L
    others = sorted(later, key=lambda k: k)[:n_other] if n_other else []
    order = sorted(list(take) + list(others))
    offs = [0]; sel = []
    for k in order:
        o0 = int(win.feature_obs_offset[k]); nob = (take[k] + 1) if k in take else int(nfac[k]) + 1
        sel.extend(range(o0, o0 + nob)); offs.append(len(sel))
    sel = np.array(sel, dtype=int); order = np.array(order, dtype=int)
    pick = lambda a: None if a is None else a[sel]
    out = abi.Window(win.para_pose, win.para_speed_bias, win.para_ex_pose, win.para_feature[order], win.feature_const[order], start[order], np.array(offs, dtype=np.int32),
                     win.obs_point[sel], win.imu, win.lidar, para_td=win.para_td, marginalization_flag=win.marginalization_flag,
                     obs_velocity=pick(win.obs_velocity), obs_cur_td=pick(win.obs_cur_td), obs_row=pick(win.obs_row), gauge_R0=win.gauge_R0, gauge_P0=win.gauge_P0)
    assert frame0_counts(out) == (mf, sum(track_lengths))
    return out


# ---- priors -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _block(win, bid, rng):
    if bid < NF:
        x0 = win.para_pose[bid].copy(); x0[:3] += rng.normal(0, 0.02, 3)
        q = synth.q_mul(x0[3:], synth.q_exp(rng.normal(0, 0.003, 3))); x0[3:] = q / np.linalg.norm(q)
        return 7, x0, np.full(6, 1e4 if bid == 0 else 1e2)
    if bid < 2 * NF:
        x0 = win.para_speed_bias[bid - NF] + np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.002, 3), rng.normal(0, 0.0002, 3)])
        return 9, x0, np.array([400.0] * 3 + [2500.0] * 3 + [2.5e5] * 3)
    return 7, win.para_ex_pose.copy(), np.full(6, 1e6)


def _table(win, ids, rng):
    blocks, diag, idx = [], [], 0
    for bid in ids:
        size, x0, d = _block(win, bid, rng)
        blocks.append(dict(id=bid, size=size, idx=idx, x0=x0)); diag.append(d); idx += len(d)
    return blocks, np.concatenate(diag)


def make_prior_over(seed, win, ids):
    """a dense full-rank prior over the blocks `ids` (in the manner of synth.make_synthetic_prior): block weights plus random couplings, J0 = chol^T, small r0"""
    rng = np.random.default_rng(seed)
    blocks, d = _table(win, ids, rng)
    n = len(d)
    Lam = np.diag(d)
    for _ in range(30):
        a = np.zeros(n)
        i, j = rng.choice(len(blocks), 2, replace=False)
        for k in (i, j):
            lo = blocks[k]["idx"]; hi = lo + (6 if blocks[k]["size"] == 7 else 9)
            a[lo:hi] = rng.normal(0, 1, hi - lo)
        Lam += rng.uniform(10, 300) * np.outer(a, a)
    return abi.make_prior(np.linalg.cholesky(Lam).T, rng.normal(0, 0.3, n), blocks)


def make_spectrum_prior(seed, win, ids, drop_id, spectrum):
    """a prior whose Schur complement on everything but block `drop_id` has the eigenvalues `spectrum`: in (dropped, kept) column order J0 = [[Ld, X], [0, S^1/2 V^T]] with
    Ld regular and V orthogonal, so that J0^T J0 / (Ld^T Ld) = V S V^T whatever X is (up to the rounding of S^1/2 V^T: ~1e-16 |S|, far below the smallest entry used)"""
    rng = np.random.default_rng(seed)
    blocks, d = _table(win, ids, rng)
    n = len(d)
    lo = next(b["idx"] for b in blocks if b["id"] == drop_id)
    dcols = np.arange(lo, lo + 6); kcols = np.array([c for c in range(n) if c < lo or c >= lo + 6])
    k = len(kcols)
    assert len(spectrum) == k
    V = np.linalg.qr(rng.normal(size=(k, k)))[0]
    Ld = np.triu(rng.normal(0, 1, (6, 6)), 1) + np.diag(rng.uniform(8, 12, 6))
    J = np.zeros((n, n))
    J[:6, dcols] = Ld; J[:6, kcols] = rng.normal(0, 1, (6, k)); J[6:, kcols] = np.sqrt(np.asarray(spectrum, dtype=float))[:, None] * V.T
    return abi.make_prior(J, rng.normal(0, 0.3, n), blocks)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; opt: overrides of the default options; build(options) -> (window, prior); env: the test hooks set for the marginalization; expected frame-0 counts mf, f0
    (None: whatever the window has), kept dimension n, and paths — amm: 'arrow' | 'jacobi', kept: 'chol' | 'eig'; source: the case whose window this one re-uses"""

    def __init__(self, name, build, opt=None, env=(), mf=None, f0=None, n=None, md=None, amm="arrow", kept="chol", rank_deficient=False, near_cut=None, source=None):
        self.name, self.build, self.opt, self.env = name, build, dict(opt or {}), tuple(env)
        self.mf, self.f0, self.n, self.md, self.amm, self.kept, self.rank_deficient = mf, f0, n, md, amm, kept, rank_deficient
        self.near_cut = near_cut          # (lo, hi): the one kept eigenvalue placed next to the 1e-8 cut on purpose (marg_reference.exact_prior_products)
        self.source = source or name

    def options(self, base):
        o = abi.Options.from_buffer_copy(bytes(base))
        for k, v in self.opt.items():
            setattr(o, k, v)
        return o

    def __repr__(self):
        return self.name


EXACT, NO_CHOL, QL = "VILF_MARG_FORCE_EXACT", "VILF_MARG_NO_CHOL", "VILF_MARG_FORCE_QL_FALLBACK"
NOLIDAR = dict(use_lidar_const=0)


def _plain(seed, n_features, flag=abi.MARGIN_OLD, tempered=True, with_prior=True):
    def build(o):
        win, prior, _ = synth.make_window(seed, o, synth.SynthConfig(with_prior=with_prior, n_features=n_features, marginalization_flag=flag))
        return (temper(win) if tempered else win), prior
    return build


def _shaped(seed, pool, mf, f0=None, n_other=30, prior_ids=None, max_len=None, with_prior=True, td=False, ex=False, imu_off=False):
    def build(o):
        win, prior, _ = synth.make_window(seed, o, synth.SynthConfig(with_prior=with_prior and prior_ids is None, n_features=pool))
        temper(win)
        if td:
            win = synth.with_td_inputs(win, seed + 1)
        if ex:
            rng = np.random.default_rng(seed + 2)
            e = win.para_ex_pose.copy(); e[:3] += rng.normal(0.0, 0.01, 3)
            q = synth.q_mul(e[3:], synth.q_exp(rng.normal(0.0, np.deg2rad(0.3), 3))); e[3:] = q / np.linalg.norm(q)
            win.para_ex_pose = e
        if imu_off:
            win.imu[1, 0] = 12.0                                        # sum_dt > 10: the reference skips IMUFactor[1] (estimator.cpp:745, :896)
        lengths = None
        if max_len is not None:
            lengths = [1 + i % max_len for i in range(mf)]
        w = shape_window(win, mf, f0, lengths, n_other) if mf is not None else win
        if prior_ids is not None:
            prior = make_prior_over(seed + 3, w, prior_ids)
        return w, prior
    return build


def _spectrum(seed, smallest):
    ids = [6, 7, 8, 9, 2 * NF]                                          # Pose[6 .. 9] and Ex_Pose; SECOND_NEW drops Pose[9]: kept dimension 24

    def build(o):
        win, _, _ = synth.make_window(seed, o, synth.SynthConfig(with_prior=False, n_features=40, marginalization_flag=abi.MARGIN_SECOND_NEW))
        temper(win)
        return win, make_spectrum_prior(seed + 3, win, ids, 9, [smallest] + list(np.logspace(0.0, 4.0, 23)))
    return build


def _cases():
    C = []
    # a. path matrix: Amm fast / forced exact x kept block Cholesky tiles / eigen / QL fallback x MARGIN_OLD / SECOND_NEW, windows of 50 and 120 features
    for seed, nfeat in ((7, 50), (22, 120)):
        for flag, ftag in ((abi.MARGIN_OLD, "old"), (abi.MARGIN_SECOND_NEW, "2nd")):
            src = f"a-{nfeat}-{ftag}"
            for amm, e1 in (("arrow", ()), ("jacobi", (EXACT,))):
                for ktag, kept, e2 in (("chol", "chol", ()), ("eig", "eig", (NO_CHOL,)), ("ql", "eig", (NO_CHOL, QL))):
                    first = amm == "arrow" and ktag == "chol"
                    C.append(Case(src if first else f"{src}-{amm}-{ktag}", _plain(seed, nfeat, flag), env=e1 + e2, n=69, md=21 if flag == abi.MARGIN_OLD else 6,
                                  amm=amm, kept=kept, source=src))
    # b. dropped-feature count: the 16-row chunks of the fast path; m = 21 + mf across MG_MLDS = 136 with the padding of odd m, fast and Jacobi (LDS / global memory)
    for mf in (0, 1, 15, 16, 17, 32, 33, 114, 115, 116, 117):
        C.append(Case(f"b-mf{mf}", _shaped(101, 460, mf), mf=mf, md=21))
        if mf >= 114:
            C.append(Case(f"b-mf{mf}-jacobi", _shaped(101, 460, mf), env=(EXACT,), mf=mf, md=21, amm="jacobi", source=f"b-mf{mf}"))
    # c. frame-0 factor count: the MG_GCH = 80 chunks of the pair gather, the MG_SLOTS = 1024 table
    for f0 in (79, 80, 81, 160, 161):
        C.append(Case(f"c-f{f0}", _shaped(102, 300, 20, f0), mf=20, f0=f0, md=21))
    for f0 in (1023, 1024, 1025):
        C.append(Case(f"c-f{f0}", _shaped(103, 760, 104, f0, n_other=10), mf=104, f0=f0, n=69, md=21))
    # d / e. md = 15 (Pose[1] stays) and the kept dimensions: 75, 76 with td (with and without the extrinsic), a small one
    C.append(Case("d-md15", _shaped(104, 120, 33, max_len=10), opt=NOLIDAR, mf=33, n=75, md=15))
    C.append(Case("d-md15-jacobi", _shaped(104, 120, 33, max_len=10), opt=NOLIDAR, env=(EXACT,), mf=33, n=75, md=15, amm="jacobi", source="d-md15"))
    C.append(Case("e-td76", _shaped(105, 160, 40, td=True, max_len=10), opt=dict(NOLIDAR, estimate_td=1), mf=40, n=76, md=15))
    C.append(Case("e-td76-ex", _shaped(106, 160, 40, td=True, ex=True, max_len=10), opt=dict(NOLIDAR, estimate_td=1, estimate_extrinsic=1), mf=40, n=76, md=15))
    C.append(Case("e-td76-eig", _shaped(105, 160, 40, td=True, max_len=10), opt=dict(NOLIDAR, estimate_td=1), env=(NO_CHOL,), mf=40, n=76, md=15, kept="eig", source="e-td76"))
    C.append(Case("e-small", _shaped(107, 200, 12, max_len=3, prior_ids=[0, 1, NF, 2 * NF]), mf=12, n=27, md=21))
    # f. truncation and guards
    C.append(Case("f-null", _shaped(108, 120, 20, prior_ids=list(range(10)) + [2 * NF], imu_off=True), mf=20, n=54, md=21, amm="jacobi"))
    C.append(Case("f-spec3e-8", _spectrum(109, 3e-8), n=24, md=6, kept="chol", near_cut=(2.9e-8, 3.1e-8)))
    C.append(Case("f-spec3e-9", _spectrum(109, 3e-9), n=24, md=6, kept="eig", rank_deficient=True, near_cut=(2.9e-9, 3.1e-9)))
    for seed in (110, 111):
        C.append(Case(f"f-gauge{seed}", _shaped(seed, 300, 60, max_len=3, with_prior=False), mf=60, n=27, md=21, kept="eig", rank_deficient=True))
    # default covariance (Amm up to 2.5e14): the same rule gives a looser bound
    for seed, nfeat in ((7, 50), (22, 120)):
        C.append(Case(f"x-default{nfeat}", _plain(seed, nfeat, tempered=False), n=69, md=21))
        C.append(Case(f"x-default{nfeat}-jacobi", _plain(seed, nfeat, tempered=False), env=(EXACT,), n=69, md=21, amm="jacobi", source=f"x-default{nfeat}"))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SOURCES = [c for c in CASES if c.source == c.name]

# g. batch shape: one upload of windows with 3, 40, 150 and 400 features (the Fmax / FACmax strides), and 65 windows tiled from 5 (two-class launches: B > 64)
RAGGED = [Case(f"g-ragged{nf}", _plain(120 + k, nf), md=21) for k, nf in enumerate((3, 40, 150, 400))]
TILED = [Case(f"g-tiled{k}", _plain((130, 131, 132, 135, 134)[k], 40), n=69, md=21) for k in range(5)]


# h. refusals
def second_new_without_its_pose(o):
    """MARGIN_SECOND_NEW with a prior that lacks Pose[WINDOW_SIZE - 1]: the prior stays as it is (estimator.cpp:982-983)"""
    win, _, _ = synth.make_window(140, o, synth.SynthConfig(with_prior=False, n_features=40, marginalization_flag=abi.MARGIN_SECOND_NEW))
    return temper(win), make_prior_over(141, win, list(range(9)) + [NF, 2 * NF])


def prior_with_a_late_speed_bias(o):
    """a prior that carries SpeedBias[3] (id NF + 3): outside what the marginalization kernels lay out"""
    win, _, _ = synth.make_window(142, o, synth.SynthConfig(with_prior=False, n_features=40))
    return temper(win), make_prior_over(143, win, [0, 2, 4, NF, NF + 3, 2 * NF])
