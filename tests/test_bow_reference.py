"""Candidate retrieval without a GPU: the vocabulary loader, the ctypes mirrors against the C layout, and tests/bow_reference.py (the restatement the kernels are
compared with in tests/test_bow.py) pinned against things that are not itself: its scores against 1 - 0.5 ||v - w||_1 in exact rational arithmetic, its transform
against a numpy search over all children at every level, its filter and its decision against the reference's lines."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction
import numpy as np
import pytest
import bow_cases as bc
import bow_reference as br
from vil_fusion_amd import abi
from vil_fusion_amd.estimator import load_vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def voc():
    return bc.tree(11, k=6, L=3)


@pytest.fixture(scope="module")
def driven(voc):
    """a revisit drive through the restatement, one detect_loop per key frame -> (frames, database, results)"""
    frames = bc.drive(5, voc, n_kf=120, n_desc=40)
    db = br.Database(voc)
    res = [db.detect_loop(f, i, max_results=16) for i, f in enumerate(frames)]
    return frames, db, res


# ---- the loader ------------------------------------------------------------------------------------------------------------------
def test_loader_round_trip(tmp_path, voc):
    path = tmp_path / "voc.bin"
    raw = bc.vocabulary_bytes(voc)
    assert len(raw) == 24 + 48 * len(voc["nodes"]) + 8 * len(voc["words"])
    path.write_bytes(raw)
    got = load_vocabulary(str(path))
    assert (got["k"], got["L"], got["scoringType"], got["weightingType"]) == (voc["k"], voc["L"], voc["scoringType"], voc["weightingType"])
    for name in ("nodeId", "parentId", "descriptor"):
        assert np.array_equal(got["nodes"][name], voc["nodes"][name]), name
    assert np.array_equal(got["nodes"]["weight"].view(np.uint64), voc["nodes"]["weight"].view(np.uint64))
    assert np.array_equal(got["words"]["nodeId"], voc["words"]["nodeId"]) and np.array_equal(got["words"]["wordId"], voc["words"]["wordId"])
    assert got["nodes"].flags.writeable and abi.BOW_NODE_DTYPE.itemsize == C.sizeof(abi.BowNode) == 48 and abi.BOW_WORD_DTYPE.itemsize == C.sizeof(abi.BowWord) == 8


@pytest.mark.parametrize("cut", [0, 23, 24 + 47, -1, -8])
def test_loader_refuses_a_truncated_file(tmp_path, voc, cut):
    raw = bc.vocabulary_bytes(voc)
    path = tmp_path / "short.bin"
    path.write_bytes(raw[:cut] if cut >= 0 else raw[:len(raw) + cut])
    with pytest.raises(ValueError):
        load_vocabulary(str(path))


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.BOW_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d %d %d\\n", VILF_BOW_MAX_DEPTH, VILF_BOW_MAX_RESULTS, VILF_BOW_LDS_WORDS);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(checks) + 3
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out) if int(o) != e]
    assert not bad, bad
    consts = [int(v) for v in out[-3:]]
    assert consts == [abi.VILF_BOW_MAX_DEPTH, abi.VILF_BOW_MAX_RESULTS, abi.VILF_BOW_LDS_WORDS] == [br.MAX_DEPTH, br.MAX_RESULTS, br.LDS_WORDS]


# ---- the restatement against something that is not itself ----------------------------------------------------------------------
def exact_score(v, w):
    """1 - 0.5 ||v - w||_1 over the fp64 vectors as they are, in rational arithmetic -> (score, common words)"""
    a, b = dict(zip(*v)), dict(zip(*w))
    l1 = sum((abs(Fraction(a.get(k, 0.0)) - Fraction(b.get(k, 0.0))) for k in set(a) | set(b)), Fraction(0))
    return 1 - l1 / 2, len(set(a) & set(b))


def test_scores_against_the_exact_l1_distance(driven):
    """Score = -s / 2 against 1 - 0.5 ||v - w||_1. The bound is derived, not measured: with c common words at most (c + 5) 2^-52. The three roundings of a term
    contribute at most 12 u in total over all terms because sum(q + d) <= 2, the c - 1 accumulating additions on partial sums of at most 2 contribute 2 (c - 1) u,
    u = 2^-53, the halving is exact. (The derivation takes ||v||_1 = ||w||_1 = 1; the normalised vectors miss that by a few u, which the 5 has covered on every
    pair here: the largest error seen is printed in units of the bound.)"""
    frames, db, res = driven
    worst, checked = 0.0, 0
    for f, r in enumerate(res):
        for e, score in r["ret"]:
            exact, c = exact_score(db.entries[f], db.entries[e])
            err = abs(Fraction(score) - exact)
            bound = Fraction(c + 5, 1 << 52)
            worst = max(worst, float(err / bound))
            assert c >= 1 and err <= bound, (f, e, c, float(err), float(bound))
            checked += 1
    print(f"{checked} scores, largest error {worst:.3f} of the bound")
    assert checked > 300


def numpy_transform(voc, desc):
    """the best child at every level by a search over all of them: distances with unpackbits, the first minimum with argmin"""
    nodes = voc["nodes"]
    bits = np.unpackbits(np.ascontiguousarray(nodes["descriptor"]).view(np.uint8).reshape(len(nodes), 32), axis=1)
    kids = {}
    for i, p in enumerate(nodes["parentId"]):
        kids.setdefault(int(p), []).append(i)                     # positions in the node array, in file order
    word = {int(r["nodeId"]): int(r["wordId"]) for r in voc["words"]}
    f = np.unpackbits(np.asarray(desc, dtype=np.uint64).view(np.uint8))
    at = 0
    while at in kids:
        rows = kids[at]
        d = (bits[rows] != f).sum(axis=1)
        best = rows[int(np.argmin(d))]
        at = int(nodes["nodeId"][best])
    i = int(np.flatnonzero(nodes["nodeId"] == at)[0])
    return word[at], float(nodes["weight"][i])


@pytest.mark.parametrize("shuffle", [False, True])
def test_transform_against_a_search_over_every_child(shuffle):
    voc = bc.tree(21, k=4, L=3, flips=3, shuffle=shuffle)         # 3 flips: siblings two to six bits apart, ties are common
    V = br.Vocabulary(voc)
    rng = np.random.default_rng(3)
    leaves = bc.leaf_descriptors(voc)
    descs = np.concatenate([bc.keyframe(rng, leaves, 200, noise=8), bc.rand_desc(rng, 100), leaves])
    ties = 0
    for d in descs:
        want = numpy_transform(voc, d)
        assert V.transform(br.as_int(d)) == want
        f = br.as_int(d)
        first = sorted(br.distance(f, V.desc[c]) for c in V.children[0])
        ties += first[0] == first[1]
    assert ties > 0                                               # a tie at the first level took place


# ---- the filter (TemplatedDatabase.h:679) ---------------------------------------------------------------------------------------
def test_filter_at_frames_48_to_52(voc):
    rng = np.random.default_rng(9)
    leaves = bc.leaf_descriptors(voc)
    shared = leaves[:5]                                           # every key frame sees five words in common
    db = br.Database(voc)
    for i in range(53):
        db.add(np.concatenate([shared, bc.keyframe(rng, leaves, 10)]))
    for f, want in ((48, [47]), (49, list(range(49))), (50, [49]), (51, [0, 50]), (52, [0, 1, 51])):
        ret = br.query_l1(db.entries[:f], db.entries[f], 0, f - 50)      # max_results 0: no cut (:712)
        assert sorted(e for e, _ in ret) == want, f
        cut = br.query_l1(db.entries[:f], db.entries[f], 4, f - 50)
        assert cut == ret[:4]


# ---- the decision (pose_graph.cpp:351-387) --------------------------------------------------------------------------------------
def test_both_thresholds_are_strict(driven):
    frames, db, res = driven
    hit = next(f for f, r in enumerate(res) if r["loop_index"] != -1)
    ret = res[hit]["ret"]
    s0, s1 = ret[0][1], max(s for _, s in ret[1:])
    base = dict(br.DEFAULTS, max_results=16)
    assert br.decide(ret, hit, base) == (True, res[hit]["loop_index"])
    assert br.decide(ret, hit, dict(base, neighbour_score=s0)) == (False, -1)
    assert br.decide(ret, hit, dict(base, neighbour_score=math.nextafter(s0, -math.inf)))[0] is True
    assert br.decide(ret, hit, dict(base, loop_score=s1)) == (False, -1)
    found, idx = br.decide(ret, hit, dict(base, loop_score=math.nextafter(s1, -math.inf)))
    assert found is True and idx != -1
    assert br.decide(ret, 50, base) == (True, -1) and br.decide(ret, 51, base)[1] != -1      # frame_index > 50, strict as well


def test_min_index_is_seeded_by_ret0_whatever_its_score():
    p = dict(br.DEFAULTS, neighbour_score=0.005)
    assert br.decide([(80, 0.01), (30, 0.5)], 100, p) == (True, 30)
    assert br.decide([(5, 0.01), (30, 0.5)], 100, p) == (True, 5)            # ret[0] below loop_score stays: nothing lower clears it
    assert br.decide([(80, 0.01), (30, 0.5), (20, 0.01)], 100, p) == (True, 30)      # a lower id below loop_score does not take over
    assert br.decide([(80, 0.01), (30, 0.01)], 100, p) == (False, -1)
    assert br.decide([(80, 0.5)], 100, p) == (False, -1)                     # the neighbour alone is no loop


def test_repeated_addition_is_not_a_product():
    """the fact the GPU tests of the vector stand on"""
    for w, c in ((0.1, 300), (math.log(1000 / 7), 65)):
        s = w
        for _ in range(c - 1):
            s = s + w
        assert s != c * w, (w, c)
    s = 0.1
    for _ in range(299):
        s += 0.1
    assert s == 30.000000000000156
