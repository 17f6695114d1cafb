"""An independent statement of the LiDAR front end, for the tests of vilf_feat.hip and of oracle/lidar_features.cpp.

Written from the text of featureExtraction.hpp:54-232 (getLaserCloud, featureExtractionFromSector, featureEdge_Surf), common.h:59-62
(DistanceXY, pointDistance) and feature_tracker_node.cpp:54-163 (getFeatureDepth), not from the oracle or the kernels. Plain numpy:
float32 arrays where the reference computes in float, float64 where it computes in double, one numpy operation (= one rounding) per
arithmetic operation of the text. That float / double mix is the contract stated in include/vilfusion.h.

Two things the text leaves open are defined as the project defines them: exactly equal curvatures sort by point index, and the three
nearest depth points are the smallest (float squared distance, index) triples of an exact search (the text asks a kd-tree).

Besides the clouds, everything a test needs to prove that a designed input hits what it was designed for is returned: rings,
curvatures, the picks of every sector and the exit every depth feature left by. ring_exact() is the ring in 40-digit arithmetic
together with the distance of the point to the nearest decision, for the probes around the ring boundaries."""
import math

import numpy as np

F = np.float32
D = np.float64


# ---------------------------------------------------------------------------------------------------------------- ring assignment
def ring_t(points, n_scans):
    """(dxy float32, angle float64, t float64, base int): t is the value the text truncates, base what it adds to the truncated
    value (N_SCANS / 2 in the lower block of the 64-ring model, else 0). No gate applied."""
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        dxy = np.sqrt(x * x + y * y)                                  # DistanceXY returns float: float products, float sum, float root
        assert dxy.dtype == F
        distance = dxy.astype(D)
        angle = np.arctan(z.astype(D) / distance) * D(180) / D(math.pi)
        base = np.zeros(len(p), dtype=np.int64)
        if n_scans == 16:
            t = (angle + D(15)) / D(2) + D(0.5)
        elif n_scans == 32:
            t = (angle + D(92.0) / D(3.0)) * D(3.0) / D(4.0)
        elif n_scans == 64:
            upper = angle >= D(-8.83)
            t = np.where(upper, (D(2) - angle) * D(3.0) + D(0.5), (D(-8.83) - angle) * D(2.0) + D(0.5))
            base = np.where(upper, 0, n_scans // 2)
        else:
            raise ValueError(n_scans)
    return dxy, angle, t, base


def ring_of(points, n_scans=64, min_r=3.0, max_r=100.0):
    """getLaserCloud's scan id per point, -1 for a point that takes one of the `continue`s. A NaN angle is a rejection (the text
    converts it to int, which C++ leaves undefined; the project defines it)."""
    dxy, angle, t, base = ring_t(points, n_scans)
    with np.errstate(all="ignore"):
        distance = dxy.astype(D)
        out = (distance < D(min_r)) | (distance > D(max_r)) | np.isnan(angle)
        idt = np.trunc(t) + base                                      # int(): toward zero, so t in (-1, 0) is scan 0
        out |= ~np.isfinite(idt) | (idt > n_scans - 1) | (idt < 0)
        if n_scans == 64:
            out |= (angle > D(2)) | (angle < D(-24.33))
    return np.where(out, -1, np.where(out, 0, idt)).astype(np.int32)


def ring_exact(points, n_scans=64, min_r=3.0, max_r=100.0, digits=40):
    """(ring int32[n], dist float64[n], terr float64[n]) in mpmath at `digits` digits. dxy is the float32 value (defined arithmetic);
    behind it angle = atan(z / dxy) * 180 / pi and t, the value that is truncated, are exact. The constants of the text are the
    doubles a compiler makes of them. dist is the distance, in units of t, to the nearest decision: an integer value of t, or one
    of the cuts of the 64-ring model (-8.83, 2, -24.33: the angle's distance times the slope of t in the point's branch).
    terr is |t_double - t_exact| of the numpy double evaluation above. Finite points inside the range gate only."""
    import mpmath as mp
    p = np.ascontiguousarray(points, dtype=F).reshape(-1, 4)
    dxy, _, td, _ = ring_t(p, n_scans)
    z = p[:, 2]
    ring = np.zeros(len(p), dtype=np.int32); dist = np.zeros(len(p)); terr = np.zeros(len(p))
    with mp.workdps(digits):
        k180pi = mp.mpf(180) / mp.pi
        half = mp.mpf(1) / 2
        c883, c2433, c923 = mp.mpf(float(D(-8.83))), mp.mpf(float(D(-24.33))), mp.mpf(float(D(92.0) / D(3.0)))
        for i in range(len(p)):
            d = float(dxy[i])
            assert math.isfinite(float(z[i])) and min_r <= d <= max_r and d > 0, (i, p[i])
            angle = mp.atan(mp.mpf(float(z[i])) / mp.mpf(d)) * k180pi
            cuts, base, rej = [], 0, False
            if n_scans == 16:
                t = (angle + 15) / 2 + half
            elif n_scans == 32:
                t = (angle + c923) * 3 / 4
            elif n_scans == 64:
                if angle >= c883:
                    t = (2 - angle) * 3 + half; slope = 3
                else:
                    t = (c883 - angle) * 2 + half; slope = 2; base = 32
                cuts = [abs(angle - c883) * slope, abs(angle - 2) * slope, abs(angle - c2433) * slope]
                rej = angle > 2 or angle < c2433
            else:
                raise ValueError(n_scans)
            idt = base + int(t)                                        # int() of an mpf truncates toward zero
            ring[i] = -1 if rej or idt > n_scans - 1 or idt < 0 else idt
            dist[i] = float(min([abs(t - mp.nint(t))] + cuts))
            terr[i] = float(abs(mp.mpf(float(td[i])) - t))
    return ring, dist, terr


# ------------------------------------------------------------------------------------------------------------- feature extraction
def _second_difference(a):
    """featureExtraction.hpp:181-189 for one coordinate: float, left to right"""
    n = len(a)
    j = np.arange(5, n - 5)
    s = a[j - 5] + a[j - 4]
    s = s + a[j - 3]
    s = s + a[j - 2]
    s = s + a[j - 1]
    s = s - F(10) * a[j]
    for k in range(1, 6):
        s = s + a[j + k]
    assert s.dtype == F
    return s


def _gap2(c, a, b):
    """squared distance of ring points a, b as :140-143: float differences, double squares and sum"""
    dx = D(c[a, 0] - c[b, 0]); dy = D(c[a, 1] - c[b, 1]); dz = D(c[a, 2] - c[b, 2])
    return dx * dx + dy * dy + dz * dz


def extract(points, n_scans=64, min_r=3.0, max_r=100.0, edge_thr=0.1):
    """extractFeature. Returns a dict:
      edge, surf   float32 (k, 4) clouds in the order of the text (rings, sectors, pick order / ascending curvature)
      rings        int32 per input point
      curv         {ring: float64 curvature of ring-local indices 5 .. cnt - 6}
      sectors      one dict per sector that was processed: ring, sector, m (elements sorted), edges (ring-local indices in pick order),
                   lost (the index of the 21st pick or None), fwd / bwd (neighbours suppressed after / before each pick, the 21st has
                   none), by_threshold (the walk ended at a value <= edge_thr), ties (adjacent equal values in the sorted sector),
                   surf (ring-local indices), first / last / dropped (ring-local index of the first, last kept and dropped element)"""
    pts = np.ascontiguousarray(points, dtype=F).reshape(-1, 4)
    rings = ring_of(pts, n_scans, min_r, max_r)
    edge, surf, sectors, curv_of = [], [], [], {}
    thr = D(edge_thr)
    for r in range(n_scans):
        c = pts[rings == r]                                            # push_back in input order
        if len(c) < 131:
            continue
        smooth_size = len(c) - 5
        dx, dy, dz = (_second_difference(c[:, k]).astype(D) for k in range(3))
        value = dx * dx + dy * dy + dz * dz                            # double, left to right
        curv_of[r] = value
        curvature = [(float(value[j - 5]), j) for j in range(5, smooth_size)]      # (value, ind)
        cloud_size = smooth_size - 5
        for s in range(6):
            length = cloud_size // 6
            start = length * s
            end = length * (s + 1) - 1
            if s == 5:
                end = cloud_size - 1
            sub = sorted(curvature[start:end], key=lambda e: (e[0], e[1]))         # [begin + start, begin + end): `end` is left out
            rec = dict(ring=r, sector=s, m=len(sub), edges=[], lost=None, fwd=[], bwd=[], by_threshold=False,
                       ties=sum(1 for a, b in zip(sub, sub[1:]) if a[0] == b[0]), first=5 + start, last=5 + end - 1, dropped=5 + end)
            picked = []                                                # cloudNeighborPicked: a list searched with std::find
            largest = 0
            for i in range(len(sub) - 1, -1, -1):
                ind = sub[i][1]
                if ind in picked:
                    continue
                if sub[i][0] <= thr:
                    rec["by_threshold"] = True
                    break
                largest += 1
                picked.append(ind)
                if largest <= 20:
                    edge.append(c[ind]); rec["edges"].append(ind)
                else:
                    rec["lost"] = ind
                    break
                nf = 0
                for k in range(1, 6):
                    if _gap2(c, ind + k, ind + k - 1) > D(0.05):
                        break
                    picked.append(ind + k); nf += 1
                nb = 0
                for l in range(-1, -6, -1):
                    if _gap2(c, ind + l, ind + l + 1) > D(0.05):
                        break
                    picked.append(ind + l); nb += 1
                rec["fwd"].append(nf); rec["bwd"].append(nb)
            rec["surf"] = [e[1] for e in sub if e[1] not in picked]
            rec["picked"] = picked
            surf.extend(c[j] for j in rec["surf"])
            sectors.append(rec)
    as_cloud = lambda l: np.array(l, dtype=F).reshape(-1, 4)
    return dict(edge=as_cloud(edge), surf=as_cloud(surf), rings=rings, curv=curv_of, sectors=sectors)


# -------------------------------------------------------------------------------------------------------------------- feature depth
def depth_threshold():
    bin_res = F(D(180.0) / D(F(360)))                                  # float bin_res = 180.0 / (float)num_bins
    return F((math.sin(float(D(bin_res) / D(180.0) * D(math.pi))) * 5.0) ** 2)


def feature_depth(cloud, feats):
    """getFeatureDepth. Returns (depth float32[m], exits list[m], clamps list[m]); exits name the way each feature left:
    few (cloud below 10 points), no3 (fewer than 3 points with a distance), threshold (third distance not below the threshold),
    spread (max - min range > 2), s_small (s <= 0.5), low (z * s not above 2), ok. clamps: "max", "min" or None."""
    c = np.ascontiguousarray(cloud, dtype=F).reshape(-1, 4)
    f = np.ascontiguousarray(feats, dtype=F).reshape(-1, 3)
    m = len(f)
    depth = np.full(m, -1.0, dtype=F); exits = ["few"] * m; clamps = [None] * m
    with np.errstate(all="ignore"):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        rng = np.sqrt(x * x + y * y + z * z)                           # pointDistance: float
        ux, uy, uz = x / rng, y / rng, z / rng
        if len(c) < 10:
            return depth, exits, clamps
        thr = depth_threshold()
        for i in range(m):
            vx, vy, vz = f[i]
            nrm = np.sqrt(vx * vx + vy * vy + vz * vz)
            vx, vy, vz = vx / nrm, vy / nrm, vz / nrm
            ex, ey, ez = ux - vx, uy - vy, uz - vz
            d = ex * ex + ey * ey + ez * ez
            assert d.dtype == F
            cand = np.flatnonzero(d < F(3.0e38))                       # a NaN distance is no neighbour
            if len(cand) < 3:
                exits[i] = "no3"; continue
            o = cand[np.lexsort((cand, d[cand]))][:3]                  # smallest (distance, index)
            if not d[o[2]] < thr:
                exits[i] = "threshold"; continue
            r1, r2, r3 = rng[o[0]], rng[o[1]], rng[o[2]]
            A = np.array([ux[o[0]] * r1, uy[o[0]] * r1, uz[o[0]] * r1], dtype=F)
            B = np.array([ux[o[1]] * r2, uy[o[1]] * r2, uz[o[1]] * r2], dtype=F)
            C = np.array([ux[o[2]] * r3, uy[o[2]] * r3, uz[o[2]] * r3], dtype=F)
            a, b = A - B, B - C
            N = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
            s = (N[0] * A[0] + N[1] * A[1] + N[2] * A[2]) / (N[0] * vx + N[1] * vy + N[2] * vz)
            assert type(s) is F
            mn, mx = min(r1, min(r2, r3)), max(r1, max(r2, r3))
            if mx - mn > 2:
                exits[i] = "spread"; continue
            if s <= 0.5:
                exits[i] = "s_small"; continue
            if s - mx > 0:
                s = mx; clamps[i] = "max"
            elif s - mn < 0:
                s = mn; clamps[i] = "min"
            inten = vz * s
            if inten > 2.0:
                depth[i] = inten; exits[i] = "ok"
            else:
                exits[i] = "low"
    return depth, exits, clamps
