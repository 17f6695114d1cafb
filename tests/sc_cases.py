"""Builders for the Scan Context edge tests (tests/test_scancontext_edges.py): clouds whose descriptor is known exactly, and databases with planted revisits.

A height map h[20][60] (0 = empty bin, otherwise a multiple of 1/8) becomes one point per non-zero bin at the bin's centre; for such a cloud
sc_reference.make_descriptor(cloud) == h bit for bit, so a test decides what the database holds instead of finding out. What follows from the arithmetic:
  * np.roll(h, k, axis=1) has the same ring key, bit for bit (a row's sum of multiples of 1/8 is exact in any order);
  * 2 h has the same normalised columns, bit for bit (scaling by a power of two is exact), hence the same distances to any query, and another ring key;
  * a map with h[:, 30:] == h[:, :30] has bit-equal distances, and bit-equal alignment norms, at the shifts s and s + 30 when it is the CANDIDATE (a symmetric query
    does not tie: its sums run over the columns in another order).
"""
import numpy as np

RINGS, SECTORS = 20, 60
DENSITY = 0.3


def random_heights(rng, density=DENSITY):
    """20 x 60, a share `density` of the bins filled with multiples of 1/8 in [1/8, 8)"""
    return np.where(rng.random((RINGS, SECTORS)) < density, rng.integers(1, 64, (RINGS, SECTORS)) / 8.0, 0.0)


def cloud_from_heights(h):
    """one point per non-zero bin: radius (r + 0.5) * 4, angle (s + 0.5) * 6 degrees, z = h - 2 (LIDAR_HEIGHT), as float32 xyzi"""
    h = np.asarray(h, dtype=np.float64)
    assert h.shape == (RINGS, SECTORS) and np.all(h * 8 == np.round(h * 8)) and np.all(np.abs(h) < 1024)
    ring, sec = np.nonzero(h)
    rad, ang = (ring + 0.5) * 4.0, np.deg2rad((sec + 0.5) * 6.0)
    return np.column_stack([rad * np.cos(ang), rad * np.sin(ang), h[ring, sec] - 2.0, np.ones(len(ring))]).astype(np.float32).reshape(-1, 4)


def variant(h, rot=0, thin=0.0, seed=0, scale=1.0, drop=None):
    """the place h seen again: a share `thin` of its filled bins lost (or `drop` of them; the first of a permutation chosen by `seed`, so variants of one seed are
    nested), then rotated by `rot` columns, heights times `scale` (a power of two)"""
    out = np.asarray(h, dtype=np.float64).copy()
    ring, sec = np.nonzero(out)
    gone = np.random.default_rng(seed).permutation(len(ring))[: int(round(thin * len(ring))) if drop is None else drop]
    out[ring[gone], sec[gone]] = 0.0
    return np.roll(out, rot, axis=1) * scale


def same_rings(h, rot, moves, seed):
    """h rotated by `rot` columns, then `moves` filled bins moved along their ring to an empty column: another descriptor with the same rows as multisets, hence the
    same ring key bit for bit, at a distance from h that is nowhere near a rounding error"""
    out = np.roll(np.asarray(h, dtype=np.float64), rot, axis=1).copy()
    rng = np.random.default_rng(seed)
    for _ in range(moves):
        ring, sec = np.nonzero(out)
        i = rng.integers(len(ring))
        free = np.flatnonzero(out[ring[i]] == 0.0)
        to = free[rng.integers(len(free))]
        out[ring[i], to], out[ring[i], sec[i]] = out[ring[i], sec[i]], 0.0
    return out


def symmetric(h):
    """h with its second half of columns replaced by the first: the same under a rotation by 30 columns"""
    out = np.asarray(h, dtype=np.float64).copy()
    out[:, 30:] = out[:, :30]
    return out


def database(n, seed, plants=None):
    """n height maps of random fill (any two are 0.6 to 0.7 apart, with gaps of 1e-3 and more between the distances). plants: {index: map or (source index, rot, thin)};
    a tuple plants variant(maps[source], rot, thin, seed=index) and is resolved in ascending index order, so a source may itself be a plant."""
    rng = np.random.default_rng(seed)
    maps = [random_heights(rng) for _ in range(n)]
    for i in sorted(plants or {}):
        v = plants[i]
        maps[i] = variant(maps[v[0]], v[1], v[2], seed=i) if isinstance(v, tuple) else np.asarray(v, dtype=np.float64)
    return maps
