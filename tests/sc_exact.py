"""The Scan Context distance from its definition at 60 digits (mpmath): what include/vilfusion.h states for `keys` and `distance`, i.e. the sector key :105-119,
fastAlignUsingVkey :104-125, distDirectSC :127-151 and distanceBtnScanContext :153-190 of global_fusion/include/Scancontext/Scancontext.h. Written from that text;
shares nothing with tests/sc_reference.py or vil_fusion_amd/csrc.

A descriptor comes as a float64 array of float32 values, so every entry is an integer times a power of two: sums of entries and sums of products are formed exactly
in Python integers, and only what is irrational or a quotient (norms, cosines, means) is rounded, to 60 digits. circshift(b, s) moves column c to (c + s) % 60.
"""
from fractions import Fraction
import mpmath

RINGS, SECTORS = 20, 60
MP = mpmath.mp.clone()
MP.dps = 60
NO_DIST = MP.mpf(10000000)


def _scaled_ints(d):
    """(integers [20][60], e) with d == integers * 2**-e exactly"""
    fr = [[Fraction(float(v)) for v in row] for row in d]
    assert len(fr) == RINGS and all(len(r) == SECTORS for r in fr)
    e = max(f.denominator.bit_length() - 1 for r in fr for f in r)
    return [[int(f * (1 << e)) for f in r] for r in fr], e


def _mpf(num, e):
    return MP.mpf(num) / MP.mpf(1 << e)


def sector_key(d):
    """column means"""
    m, e = _scaled_ints(d)
    return [_mpf(sum(m[r][c] for r in range(RINGS)), e) / RINGS for c in range(SECTORS)]


def align_norms(a, b):
    """[s] = |sector_key(a) - circshift(sector_key(b), s)| for the 60 shifts"""
    ka, kb = sector_key(a), sector_key(b)
    return [MP.sqrt(sum((ka[c] - kb[(c - s) % SECTORS]) ** 2 for c in range(SECTORS))) for s in range(SECTORS)]


def shift_distances(a, b):
    """[s] = distDirectSC(a, circshift(b, s)): 1 - the mean, over the columns where both norms are non-zero, of the cosine between the columns; None where there is
    no such column"""
    ma, ea = _scaled_ints(a)
    mb, eb = _scaled_ints(b)
    ca = [[ma[r][c] for r in range(RINGS)] for c in range(SECTORS)]
    cb = [[mb[r][c] for r in range(RINGS)] for c in range(SECTORS)]
    qa = [sum(v * v for v in col) for col in ca]                        # squared norms, exact (scaled by 4**e)
    qb = [sum(v * v for v in col) for col in cb]
    na = [MP.sqrt(MP.mpf(q)) for q in qa]
    nb = [MP.sqrt(MP.mpf(q)) for q in qb]
    cos = {}
    for c in range(SECTORS):
        for x in range(SECTORS):
            if qa[c] and qb[x]:
                cos[c, x] = MP.mpf(sum(u * v for u, v in zip(ca[c], cb[x]))) / (na[c] * nb[x])       # the scale 2**-(ea + eb) cancels
    out = []
    for s in range(SECTORS):
        terms = [cos[c, (c - s) % SECTORS] for c in range(SECTORS) if (c, (c - s) % SECTORS) in cos]
        out.append(1 - sum(terms) / len(terms) if terms else None)
    return out


def search_window(first, radius):
    """the searched shifts in the order they are searched: ascending"""
    return sorted({(first + i) % SECTORS for i in range(-radius, radius + 1)})


def first_min(values, order, start):
    """first strict minimum below `start` over `order`; (start, None) if nothing is below it"""
    best, arg = start, None
    for s in order:
        if values[s] is not None and values[s] < best:
            best, arg = values[s], s
    return best, arg


def distance(a, b, radius, norms=None, dists=None):
    """distanceBtnScanContext -> (distance, shift, aligned shift); (10000000, 0, aligned) when no searched shift has a distance"""
    norms = align_norms(a, b) if norms is None else norms
    dists = shift_distances(a, b) if dists is None else dists
    _, al = first_min(norms, range(SECTORS), NO_DIST)
    al = 0 if al is None else al
    best, arg = first_min(dists, search_window(al, radius), NO_DIST)
    return best, (0 if arg is None else arg), al


def gap_to_runner_up(values, order):
    """second smallest minus smallest of the defined values over `order` (inf with fewer than two)"""
    v = sorted(values[s] for s in order if values[s] is not None)
    return v[1] - v[0] if len(v) > 1 else MP.inf
