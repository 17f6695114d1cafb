"""Candidate retrieval of the visual loop closure on the device (vilf_kf_bow_*, estimator.KeyFrameStore.detectLoop) against tests/bow_reference.py, the plain
Python restatement of the contract in include/vilfusion.h: every integer equal, every float equal in its bits. The restatement itself is measured in
tests/test_bow_reference.py. Key frames are descriptor sets that go in through vilf_kf_add_loaded; one case goes through the images."""
import ctypes as C
import math
import numpy as np
import pytest
import bow_cases as bc
import bow_reference as br
import kf_reference as kr
from vil_fusion_amd import abi

pytestmark = pytest.mark.gpu
CAM = (460.0, 460.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)
PATTERN = kr.read_pattern()
INV, UNS = abi.VILF_ERR_INVALID_ARGUMENT, abi.VILF_ERR_UNSUPPORTED


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, voc=None, cap_keyframes=160, cap_keypoints=1 << 15):
    from vil_fusion_amd.estimator import KeyFrameStore
    t = KeyFrameStore(solver, 64, 48, CAM, PATTERN, cap_keyframes=cap_keyframes, cap_keypoints=cap_keypoints)
    if voc is not None:
        t.set_vocabulary(voc)
    return t


def same_transform(t, V, descs, what=""):
    w, wt = t.bow_transform(descs)
    rw, rwt = V.transform_all(descs)
    assert w.dtype == np.int32 and np.array_equal(w, rw), (what, np.flatnonzero(w != rw)[:8])
    assert np.array_equal(bits(wt), bits(rwt)), what
    return rw


def same_vector(got, want, what=""):
    assert np.array_equal(got[0], np.array(want[0], dtype=np.int32)), (what, got[0][:8], want[0][:8])
    assert np.array_equal(bits(got[1]), bits(np.array(want[1], dtype=np.float64))), what


def same_result(got, want, what=""):
    for k in ("loop_index", "find_loop", "n_results", "n_words"):
        assert got[k] == want[k], (what, k, got[k], want[k], got["ret"], want["ret"])
    assert np.array_equal(got["id"], want["id"]), (what, got["id"], want["id"])
    assert np.array_equal(bits(got["score"]), bits(want["score"])), (what, got["score"], want["score"])


def grow(rng, shape, flips=16, weight=None):
    """a vocabulary from a nested shape: None is a leaf, a list an inner node with those children; ids in breadth-first order. A child's descriptor is its parent's
    with `flips` bits flipped."""
    records, level, nid = [], [(0, None, shape)], 0
    while level:
        nxt = []
        for pid, pdesc, kids in level:
            for kid in kids:
                nid += 1
                d = bc.rand_desc(rng) if pdesc is None else bc.flip(rng, pdesc, flips)
                records.append((nid, pid, bc.idf_weight(rng) if weight is None else weight, d))
                if kid is not None:
                    nxt.append((nid, d, kid))
        level = nxt
    return records


def probes(rng, records, n=120):
    """descriptors near the nodes of a vocabulary, the nodes' own descriptors and random ones"""
    own = np.array([r[3] for r in records], dtype=np.uint64)
    near = np.array([bc.flip(rng, own[i], rng.integers(0, 12)) for i in rng.integers(0, len(own), size=n)], dtype=np.uint64)
    return np.concatenate([own, near, bc.rand_desc(rng, 40)])


# ---- transform -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voc1000():
    voc = bc.tree(1, k=10, L=3)
    return voc, br.Vocabulary(voc)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 300])
def test_transform_sizes(solver, voc1000, n):
    """k = 10, L = 3, 1000 words; 16 descriptors per workgroup, four per wave"""
    voc, V = voc1000
    t = make(solver, voc)
    rng = np.random.default_rng(100 + n)
    descs = np.concatenate([bc.keyframe(rng, bc.leaf_descriptors(voc), n - n // 4, noise=10), bc.rand_desc(rng, n // 4)]) if n else np.zeros((0, 4), dtype=np.uint64)
    rw = same_transform(t, V, descs, n)
    assert len(rw) == n and (n < 63 or len(set(rw.tolist())) > 30)


def test_transform_of_the_nodes_own_descriptors(solver, voc1000):
    voc, V = voc1000
    t = make(solver, voc)
    rw = same_transform(t, V, voc["nodes"]["descriptor"])
    leaves = bc.leaf_descriptors(voc)
    assert np.array_equal(same_transform(t, V, leaves), np.arange(1000))      # a leaf's descriptor is its own word


def test_transform_ties_go_to_the_earlier_child(solver):
    """two identical children, two different children at equal distance; positions in one lane's two rounds (3 and 19) and on both sides of the group width (15, 16)"""
    rng = np.random.default_rng(7)
    rec = grow(rng, [None] * 33, weight=1.0)
    for a, b in ((3, 19), (15, 16), (0, 32)):
        rec[b] = (rec[b][0], rec[b][1], rec[b][2], rec[a][3].copy())           # identical twins
    voc = bc.assemble(rec)
    V = br.Vocabulary(voc)
    t = make(solver, voc)
    f = bc.rand_desc(rng)
    rec2 = list(rec)
    for pos, bit in ((5, 0), (21, 1), (14, 2), (17, 3)):                       # four children one bit away from f, each another bit
        d = f.copy(); d[0] ^= np.uint64(1 << bit)
        rec2[pos] = (rec2[pos][0], 0, 1.0, d)
    voc2 = bc.assemble(rec2)
    V2 = br.Vocabulary(voc2)
    twins = np.array([rec[3][3], rec[15][3], rec[0][3]], dtype=np.uint64)
    assert same_transform(t, V, twins).tolist() == [3, 15, 0]                  # words are the leaves in id order: word = position
    same_transform(t, V, probes(rng, rec))
    t2 = make(solver, voc2)
    assert same_transform(t2, V2, f.reshape(1, 4)).tolist() == [5]
    same_transform(t2, V2, probes(rng, rec2))


def test_child_order_is_the_file_order_not_the_id_order(solver):
    rng = np.random.default_rng(8)
    rec = grow(rng, [[None] * 6] * 5, weight=1.0)
    for i in range(5, len(rec), 2):                                            # every other leaf is the twin of the one before it
        if rec[i][1] == rec[i - 1][1]:
            rec[i] = (rec[i][0], rec[i][1], rec[i][2], rec[i - 1][3].copy())
    by_id = bc.assemble(rec)
    words = [(int(r["nodeId"]), int(r["wordId"])) for r in by_id["words"]]
    shuffled = bc.assemble([rec[i] for i in rng.permutation(len(rec))], words=words)
    descs = probes(rng, rec)
    a = same_transform(make(solver, by_id), br.Vocabulary(by_id), descs)
    b = same_transform(make(solver, shuffled), br.Vocabulary(shuffled), descs)
    assert (a != b).any()


def test_children_counts_around_the_group_width(solver):
    rng = np.random.default_rng(9)
    rec = grow(rng, [[None] * 1, [None] * 15, [None] * 16, [None] * 17, [None] * 33])
    voc = bc.assemble(rec)
    rw = same_transform(make(solver, voc), br.Vocabulary(voc), probes(rng, rec, 300))
    assert len(set(rw.tolist())) == 82


def test_unbalanced_tree(solver):
    """a leaf at depth 1 beside inner nodes, leaves at depths 2 and 3"""
    rng = np.random.default_rng(10)
    rec = grow(rng, [None, [None, None, [None, None, None]], None, [[None, None], None]])
    voc = bc.assemble(rec)
    V = br.Vocabulary(voc)
    rw = same_transform(make(solver, voc), V, probes(rng, rec, 200))
    assert sorted(set(V.depth[int(r["nodeId"])] for r in voc["words"])) == [1, 2, 3] and len(set(rw.tolist())) == len(voc["words"])


def chain(depth):
    shape = [None, None]
    for _ in range(depth - 1):
        shape = [None, shape]
    return shape


def test_deepest_tree(solver):
    rng = np.random.default_rng(11)
    rec = grow(rng, chain(abi.VILF_BOW_MAX_DEPTH), flips=6)
    voc = bc.assemble(rec)
    V = br.Vocabulary(voc)
    assert max(V.depth.values()) == abi.VILF_BOW_MAX_DEPTH
    rw = same_transform(make(solver, voc), V, probes(rng, rec, 200))
    deepest = [int(r["wordId"]) for r in voc["words"] if V.depth[int(r["nodeId"])] == abi.VILF_BOW_MAX_DEPTH]
    assert set(deepest) <= set(rw.tolist())


# ---- the vector ------------------------------------------------------------------------------------------------------------------
def one_word_voc(w, weighting=abi.VILF_BOW_TF_IDF):
    rng = np.random.default_rng(12)
    rec = grow(rng, [[None] * 4] * 3)
    rec = [(n, p, w if n == 4 else 0.7, d) for n, p, _, d in rec]              # node 4 is the first leaf: word 0
    return bc.assemble(rec, weighting=weighting), rec


@pytest.mark.parametrize("w,c", [(0.1, 300), (math.log(1000 / 7), 65)])
def test_a_repeated_word_is_a_repeated_addition(solver, w, c):
    voc, rec = one_word_voc(w)
    V = br.Vocabulary(voc)
    descs = np.array([rec[3][3]] * c + [rec[4][3]] * 3, dtype=np.uint64)       # c times word 0, three times word 1
    ids, vals = V.bow_vector(descs)
    s = w
    for _ in range(c - 1):
        s = s + w
    assert s != c * w and ids == [0, 1]
    t3 = (0.7 + 0.7) + 0.7
    assert vals == [s / (s + t3), t3 / (s + t3)] and vals != [c * w / (c * w + t3), t3 / (c * w + t3)]      # the product would show in the stored vector
    t = make(solver, voc)
    bc.load(t, descs)
    bc.load(t, descs[:c])                                                      # the word alone: 1.0
    t.bow_add_range(0, 2)
    same_vector(t.bow_vector(0), (ids, vals))
    same_vector(t.bow_vector(1), ([0], [1.0]))


@pytest.mark.parametrize("weighting", [abi.VILF_BOW_TF_IDF, abi.VILF_BOW_TF, abi.VILF_BOW_IDF, abi.VILF_BOW_BINARY])
def test_the_four_weightings_and_stop_words(solver, weighting):
    voc = bc.tree(2, k=5, L=3, weighting=weighting, stop_fraction=0.3)
    V = br.Vocabulary(voc)
    leaves = bc.leaf_descriptors(voc)
    stopped = [int(r["wordId"]) for r in voc["words"] if V.weight[int(r["nodeId"])] == 0.0]
    assert 20 < len(stopped) < 60
    rng = np.random.default_rng(13)
    frames = [bc.keyframe(rng, leaves, n, noise=3) for n in (1, 63, 64, 65, 257, 300, 700)]
    frames += [leaves[stopped], np.zeros((0, 4), dtype=np.uint64), leaves[stopped[:1]], bc.keyframe(rng, leaves, 90)]      # stopped words only, no key points
    t = make(solver, voc)
    for f in frames:
        bc.load(t, f)
    for i in range(len(frames)):
        t.bow_add(i)
    assert t.bow_size() == len(frames)
    for i, f in enumerate(frames):
        want = V.bow_vector(f)
        same_vector(t.bow_vector(i), want, i)
        assert len(want[0]) == 0 if i in (7, 8, 9) else len(want[0]) > 0 or i == 0      # the single descriptor of frame 0 may be a stopped word
    w700 = V.bow_vector(frames[6])
    assert len(w700[0]) < 125 and not set(w700[0]) & set(stopped)              # words repeat: the counts matter
    res = t.detect_loop_range(0, len(frames), min_gap=0, max_results=16)
    db = br.Database(V)
    for f in frames:
        db.add(f)
    for i, (g, r) in enumerate(zip(res, db.detect_loop_range(0, len(frames), min_gap=0, max_results=16))):
        same_result(g, r, i)
    assert res[8]["n_words"] == 0 and res[8]["n_results"] == 0 and all(8 not in [e for e, _ in r["ret"]] for r in res)


def test_vector_of_key_frames_from_images(solver):
    voc = bc.tree(3, k=10, L=3)
    V = br.Vocabulary(voc)
    t = make(solver, voc, cap_keyframes=4)
    rng = np.random.default_rng(14)
    for i in range(3):
        img = rng.integers(0, 256, size=(48, 64)).astype(np.uint8)            # noise: a few hundred FAST corners
        idx, nkp = t.add_keyframe(img, np.zeros((0, 2), dtype=np.float32))
        assert idx == i and nkp > 100
        assert t.detectLoop(i) == -1
    for i in range(3):
        same_vector(t.bow_vector(i), V.bow_vector(t.get(i)["descriptors"]), i)


# ---- score and select ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """a database of 115 loaded key frames over 4096 words: a drive, then the engineered vectors -> (voc, frames, reference database, marks)"""
    voc = bc.tree(4, k=8, L=4)
    V = br.Vocabulary(voc)
    leaves = bc.leaf_descriptors(voc)
    rng = np.random.default_rng(15)
    frames = bc.drive(6, voc, n_kf=100, n_desc=40, revisit_from=80, n_leaves=4000)      # the last 96 words are kept out of the drive
    W = np.sort(rng.choice(4000, size=129, replace=False))                     # the words of the 129-word entry
    other = np.setdiff1d(np.arange(4000), W)
    m = {}

    def put(name, words):
        m[name] = len(frames)
        frames.append(leaves[np.asarray(words, dtype=np.int64)] if len(words) else np.zeros((0, 4), dtype=np.uint64))
    put("e129", W)
    put("edges", np.concatenate([W[[0, 63, 64, 127, 128]], other[:20]]))       # common words on both sides of each 64-word boundary of the entry
    put("q63", W[:63]); put("q64", W[:64]); put("q65", W[1:66])
    put("empty", [])
    dup = np.concatenate([W[40:70], other[100:110]])
    put("dup0", dup); put("dup1", dup); put("dup2", dup)
    put("probe", np.concatenate([W[50:60], other[105:120]]))
    put("alone", np.arange(4000, 4010))                                        # words nobody before it has
    put("lds", np.arange(abi.VILF_BOW_LDS_WORDS))                              # as many words as the LDS copy holds
    put("global", np.arange(abi.VILF_BOW_LDS_WORDS + 1))                       # one more: read from global memory
    put("after", np.concatenate([np.arange(0, 4096, 37), W[:5]]))
    put("global2", np.arange(5, abi.VILF_BOW_LDS_WORDS + 200))
    db = br.Database(V)
    for f in frames:
        db.add(f)
    for name, n in (("e129", 129), ("q63", 63), ("q64", 64), ("q65", 65), ("empty", 0), ("lds", abi.VILF_BOW_LDS_WORDS), ("global", abi.VILF_BOW_LDS_WORDS + 1)):
        assert len(db.entries[m[name]][0]) == n, name
    return voc, frames, db, m


@pytest.fixture(scope="module")
def big_store(big):
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    voc, frames, db, m = big
    t = make(s, voc, cap_keyframes=len(frames), cap_keypoints=sum(len(f) for f in frames))      # both capacities to the brim
    for f in frames:
        bc.load(t, f)
    t.bow_add_range(0, len(frames))
    yield t
    s.close()


def test_stored_vectors_of_the_big_database(big, big_store):
    voc, frames, db, m = big
    assert big_store.bow_size() == len(frames)
    for i in (0, 50, m["e129"], m["empty"], m["lds"], m["global"], len(frames) - 1):
        same_vector(big_store.bow_vector(i), db.entries[i], i)


@pytest.mark.parametrize("max_results,min_gap", [(16, 0), (4, 50), (1, 0), (16, 50), (4, 3)])
def test_queries_over_the_big_database(big, big_store, max_results, min_gap):
    voc, frames, db, m = big
    n = len(frames)
    got = big_store.detect_loop_range(0, n, max_results=max_results, min_gap=min_gap)
    want = db.detect_loop_range(0, n, max_results=max_results, min_gap=min_gap)
    for i in range(n):
        same_result(got[i], want[i], i)
    ids = lambda name: [e for e, _ in want[m[name]]["ret"]]
    if (max_results, min_gap) == (16, 0):
        assert want[1]["n_results"] <= 1 and want[3]["n_results"] < 16                           # fewer results than max_results
        assert want[m["empty"]]["n_results"] == 0 and all(m["empty"] not in [e for e, _ in r["ret"]] for r in want)
        assert m["e129"] in ids("edges") and m["e129"] in ids("q63") and m["e129"] in ids("q64") and m["e129"] in ids("q65")
        p = want[m["probe"]]["ret"]
        k = [e for e, _ in p].index(m["dup0"])
        assert [e for e, _ in p[k:k + 3]] == [m["dup0"], m["dup1"], m["dup2"]] and p[k][1] == p[k + 1][1] == p[k + 2][1]      # equal scores in id order
        assert want[m["alone"]]["n_results"] == 0                                                 # the eligible entries share no word with it
        assert m["lds"] in ids("global") and m["global"] in ids("after") and m["global"] in ids("global2") and want[m["global"]]["n_words"] == abi.VILF_BOW_LDS_WORDS + 1
        assert want[m["global"]]["ret"][0][0] == m["lds"] and want[m["global"]]["ret"][0][1] > 0.99      # 2048 common words, summed in order
    if max_results == 1:
        assert all(r["n_results"] <= 1 for r in want) and sum(r["n_results"] for r in want) > 90
    if (max_results, min_gap) == (4, 50):
        assert [e for e, _ in want[48]["ret"]] == [47] and len(want[49]["ret"]) == 4 and [e for e, _ in want[50]["ret"]] == [49]


def test_a_replay_in_several_batches(solver, voc1000):
    """3000 key frames: their 3000 x 2999 score cells exceed the 2^23 of one batch, so the replay goes in two. The batches against pieces that need none, to the bit,
    and the last rows against the restatement."""
    voc, V = voc1000
    n = 3000
    rng = np.random.default_rng(18)
    leaves = bc.leaf_descriptors(voc)
    frames = leaves[rng.integers(0, 1000, size=(n, 3))]
    assert n * (n - 1) > 1 << 23 and 500 * (n - 1) < 1 << 23
    t = make(solver, voc, cap_keyframes=n, cap_keypoints=3 * n)
    for f in frames:
        bc.load(t, f)
    t.bow_add_range(0, n)
    whole = t.detect_loop_range(0, n)
    pieces = [r for first in range(0, n, 500) for r in t.detect_loop_range(first, 500)]
    for i, (a, b) in enumerate(zip(whole, pieces)):
        same_result(a, b, i)
    db = br.Database(V)
    for f in frames:
        db.add(f)
    for i, w in zip((1400, 1499, 1500, 1501, n - 1), (db.detect_loop_range(i, 1)[0] for i in (1400, 1499, 1500, 1501, n - 1))):
        same_result(whole[i], w, i)
        assert w["n_results"] == 4


# ---- detectLoop ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voc10k():
    voc = bc.tree(1, k=10, L=4)
    return voc, br.Vocabulary(voc)


@pytest.fixture(scope="module")
def driven(voc10k):
    """120 key frames of 100 descriptors over 10000 words; frames 100 .. revisit frames 10 .., every other one with two descriptors only"""
    voc, V = voc10k
    frames = bc.drive(5, voc)
    db = br.Database(V)
    want = [db.detect_loop(f, i) for i, f in enumerate(frames)]
    loops = [r["loop_index"] for r in want]
    shares = lambda i: bool(set(db.entries[i][0]) & set(db.entries[i - 90][0]))
    assert sum(loops[i] != -1 and abs(loops[i] - (i - 90)) <= 2 for i in range(100, 120)) >= 5     # revisits found: the lowest id of the old place's results
    assert any(loops[i] == -1 and shares(i) for i in range(100, 120))                              # a revisit that shares words and is missed by the thresholds
    assert any(r["find_loop"] and r["loop_index"] == -1 for r in want[:51]) and all(l == -1 for l in loops[:51])      # the frame_index > min_gap gate
    return frames, db, want


def test_detect_loop_and_its_replay(solver, voc10k, driven):
    """a drive of 120 key frames, frames 100 .. revisit frames 10 ..: single calls, then detect_range over the finished database, to the bit"""
    voc, V = voc10k
    frames, db, want = driven
    t = make(solver, voc)
    for i, f in enumerate(frames):
        assert bc.load(t, f) == i
        got = t.detect_loop(i)
        same_result(got, want[i], i)
        assert t.bow_size() == i + 1
    for i, g in enumerate(t.detect_loop_range(0, len(frames))):
        same_result(g, want[i], ("replay", i))
    for i, g in enumerate(t.detect_loop_range(95, 20)):
        same_result(g, want[95 + i], ("replay from 95", i))
    singles = [t.bow_vector(i) for i in range(len(frames))]
    t2 = make(solver, voc)
    for f in frames:
        bc.load(t2, f)
    t2.bow_add_range(0, 70)
    t2.bow_add_range(70, 0)
    t2.bow_add_range(70, 50)
    for i in range(len(frames)):
        same_vector(t2.bow_vector(i), singles[i], i)
        same_vector(singles[i], db.entries[i], i)


def test_thresholds_on_the_device_are_strict(solver, voc10k, driven):
    voc, V = voc10k
    frames, db, want = driven
    hit = next(i for i, r in enumerate(want) if r["loop_index"] != -1)
    t = make(solver, voc)
    for f in frames[:hit + 1]:
        bc.load(t, f)
    t.bow_add_range(0, hit + 1)
    ret = want[hit]["ret"]
    s0, s1 = ret[0][1], max(s for _, s in ret[1:])
    for over, loop in ((dict(neighbour_score=s0), False), (dict(neighbour_score=math.nextafter(s0, -math.inf)), True), (dict(loop_score=s1), False),
                       (dict(loop_score=math.nextafter(s1, -math.inf)), True), (dict(min_gap=hit), False), (dict(min_gap=hit - 1), True)):
        g = t.detect_loop_range(hit, 1, **over)[0]
        same_result(g, db.detect_loop_range(hit, 1, **over)[0], over)
        assert (g["loop_index"] != -1) == loop, over


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def broken_vocabularies():
    rng = np.random.default_rng(16)
    rec = grow(rng, [[None, None], [None, None, None]])
    good = bc.assemble(rec)
    out = {}

    def nodes(fn):
        v = dict(good, nodes=good["nodes"].copy(), words=good["words"].copy()); fn(v); return v
    out["an id twice"] = nodes(lambda v: v["nodes"]["nodeId"].__setitem__(3, 2))
    out["an id of 0"] = nodes(lambda v: v["nodes"]["nodeId"].__setitem__(3, 0))
    out["an id beyond nNodes"] = nodes(lambda v: v["nodes"]["nodeId"].__setitem__(3, 8))
    out["a parent that does not exist"] = nodes(lambda v: v["nodes"]["parentId"].__setitem__(3, 9))
    out["a negative parent"] = nodes(lambda v: v["nodes"]["parentId"].__setitem__(3, -1))
    out["its own parent"] = nodes(lambda v: v["nodes"]["parentId"].__setitem__(3, int(v["nodes"]["nodeId"][3])))

    def cycle(v):                                                              # nodes 1 and 3 hang on each other: the root reaches neither
        v["nodes"]["parentId"][0] = 3
    out["unreachable nodes"] = nodes(cycle)
    out["a leaf without a word"] = nodes(lambda v: v.__setitem__("words", v["words"][:-1]))
    out["a word on an inner node"] = nodes(lambda v: v["words"]["nodeId"].__setitem__(0, 1))
    out["a word id beyond nWords"] = nodes(lambda v: v["words"]["wordId"].__setitem__(0, 5))
    out["a negative word id"] = nodes(lambda v: v["words"]["wordId"].__setitem__(0, -1))
    out["a word id twice"] = nodes(lambda v: v["words"]["wordId"].__setitem__(0, 1))
    out["a word for a node that does not exist"] = nodes(lambda v: v["words"]["nodeId"].__setitem__(0, 99))
    out["a negative weight"] = nodes(lambda v: v["nodes"]["weight"].__setitem__(2, -0.5))
    out["a weight that is NaN"] = nodes(lambda v: v["nodes"]["weight"].__setitem__(2, np.nan))
    out["an infinite weight"] = nodes(lambda v: v["nodes"]["weight"].__setitem__(2, np.inf))
    out["too deep"] = bc.assemble(grow(rng, chain(abi.VILF_BOW_MAX_DEPTH + 1)))
    out["no nodes"] = dict(good, nodes=good["nodes"][:0], words=good["words"][:0])
    out["a weighting that does not exist"] = dict(good, weightingType=4)
    out["a scoring that does not exist"] = dict(good, scoringType=6)
    for s in range(1, 6):
        out[f"scoring {s}"] = dict(good, scoringType=s)
    return good, out


def test_refusals(solver):
    from vil_fusion_amd.estimator import BackendSolver, VilfError, bow_default_params
    good, broken = broken_vocabularies()
    V = br.Vocabulary(good)
    rng = np.random.default_rng(17)
    leaves = bc.leaf_descriptors(good)
    frames = [bc.keyframe(rng, leaves, 12) for _ in range(4)]
    t = make(solver, good, cap_keyframes=8)
    for f in frames:
        bc.load(t, f)
    t.bow_add_range(0, 2)
    L, h = t._L, solver._h
    p = bow_default_params()
    row, rows = abi.BowResult(), (abi.BowResult * 4)()
    before = t.bow_vector(1)

    def untouched(what):
        assert t.bow_size() == 2, what
        same_vector(t.bow_vector(1), before, what)
        same_vector(before, V.bow_vector(frames[1]), what)

    def pvoc(v):
        n, w = np.ascontiguousarray(v["nodes"]), np.ascontiguousarray(v["words"])
        return abi.BowVocabulary(v["k"], v["L"], v["scoringType"], v["weightingType"], len(n), len(w), n.ctypes.data_as(C.POINTER(abi.BowNode)), w.ctypes.data_as(C.POINTER(abi.BowWord))), (n, w)

    for what, v in broken.items():
        with pytest.raises(ValueError):
            br.Vocabulary(v)
        cv, keep = pvoc(v)
        assert L.vilf_kf_bow_set_vocabulary(h, C.byref(cv)) == (UNS if what.startswith("scoring ") else INV), what
        untouched(what)
    cv, keep = pvoc(good)
    for field in ("nodes", "words"):
        bad = abi.BowVocabulary.from_buffer_copy(cv)
        setattr(bad, field, None)
        assert L.vilf_kf_bow_set_vocabulary(h, C.byref(bad)) == INV, field
    assert L.vilf_kf_bow_set_vocabulary(h, None) == INV
    untouched("null vocabulary")
    desc = np.ascontiguousarray(frames[0])
    w, wt, cnt = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.float64), C.c_int(-7)
    calls = {
        "add out of order (behind)": lambda: L.vilf_kf_bow_add(h, 1),
        "add out of order (ahead)": lambda: L.vilf_kf_bow_add(h, 3),
        "add beyond the store": lambda: L.vilf_kf_bow_add_range(h, 2, 3),
        "add a negative count": lambda: L.vilf_kf_bow_add_range(h, 2, -1),
        "detect out of order": lambda: L.vilf_kf_bow_detect(h, C.byref(p), 3, C.byref(row)),
        "detect an entry": lambda: L.vilf_kf_bow_detect(h, C.byref(p), 1, C.byref(row)),
        "detect without parameters": lambda: L.vilf_kf_bow_detect(h, None, 2, C.byref(row)),
        "detect without a result": lambda: L.vilf_kf_bow_detect(h, C.byref(p), 2, None),
        "replay beyond the database": lambda: L.vilf_kf_bow_detect_range(h, C.byref(p), 1, 2, rows),
        "replay from a negative index": lambda: L.vilf_kf_bow_detect_range(h, C.byref(p), -1, 2, rows),
        "replay without results": lambda: L.vilf_kf_bow_detect_range(h, C.byref(p), 0, 2, None),
        "get beyond the database": lambda: L.vilf_kf_bow_get(h, 2, 16, t._ip(w), abi.dptr(wt), C.byref(cnt)),
        "get a negative index": lambda: L.vilf_kf_bow_get(h, -1, 16, t._ip(w), abi.dptr(wt), C.byref(cnt)),
        "get into too little room": lambda: L.vilf_kf_bow_get(h, 1, len(before[0]) - 1, t._ip(w), abi.dptr(wt), C.byref(cnt)),
        "transform without descriptors": lambda: L.vilf_kf_bow_transform(h, None, 3, t._ip(w), abi.dptr(wt)),
        "transform without outputs": lambda: L.vilf_kf_bow_transform(h, t._u64(desc), 3, None, abi.dptr(wt)),
        "transform a negative count": lambda: L.vilf_kf_bow_transform(h, t._u64(desc), -1, t._ip(w), abi.dptr(wt)),
    }
    for field, value in (("max_results", 0), ("max_results", abi.VILF_BOW_MAX_RESULTS + 1), ("min_gap", -1), ("neighbour_score", math.nan), ("loop_score", math.nan)):
        q = bow_default_params(**{field: value})
        calls[f"detect with {field} = {value}"] = lambda q=q: L.vilf_kf_bow_detect(h, C.byref(q), 2, C.byref(row))
        calls[f"replay with {field} = {value}"] = lambda q=q: L.vilf_kf_bow_detect_range(h, C.byref(q), 0, 2, rows)
    for what, call in calls.items():
        assert call() == INV, what
        assert cnt.value == -7 and not w.any() and not wt.any(), what
        untouched(what)
    assert L.vilf_kf_bow_size(h, None) == INV and L.vilf_kf_bow_profile(h, None, None) == INV
    # after all of it the database still works
    same_result(t.detect_loop(2), br.Database(V).result(*_third(V, frames)), "after the refusals")
    # no vocabulary, no store
    other = BackendSolver()
    try:
        n = C.c_int(-1)
        assert other._L.vilf_kf_bow_size(other._h, C.byref(n)) == 0 and n.value == 0
        assert other._L.vilf_kf_bow_set_vocabulary(other._h, C.byref(cv)) == INV                   # no store
        assert other._L.vilf_kf_bow_add(other._h, 0) == INV
        t3 = make(other)
        bc.load(t3, frames[0])
        for call in (lambda: other._L.vilf_kf_bow_add(other._h, 0), lambda: other._L.vilf_kf_bow_detect(other._h, C.byref(p), 0, C.byref(row)),
                     lambda: other._L.vilf_kf_bow_detect_range(other._h, C.byref(p), 0, 0, rows), lambda: other._L.vilf_kf_bow_get(other._h, 0, 16, t._ip(w), abi.dptr(wt), C.byref(cnt)),
                     lambda: other._L.vilf_kf_bow_transform(other._h, t._u64(desc), 3, t._ip(w), abi.dptr(wt))):
            assert call() == INV                                                                    # no vocabulary
        with pytest.raises(VilfError):
            t3.detectLoop(0)
        t3.set_vocabulary(good)
        assert t3.detectLoop(0) == -1 and t3.bow_size() == 1
        t3.set_vocabulary(good)                                                                     # a new vocabulary drops the database
        assert t3.bow_size() == 0
        assert other._L.vilf_reset(other._h) == 0 and t3.detectLoop(0) == -1 and t3.bow_size() == 1      # vilf_reset leaves it alone
        t4 = make(other)                                                                            # a new store drops vocabulary and database
        assert t4.bow_size() == 0 and other._L.vilf_kf_bow_add(other._h, 0) == INV
    finally:
        other.close()


def _third(V, frames):
    db = br.Database(V)
    db.add(frames[0]); db.add(frames[1])
    r = db.detect_loop(frames[2], 2)
    return (db.entries[2], r["ret"], 2, br.DEFAULTS)


# ---- the pose graph --------------------------------------------------------------------------------------------------------------
class Recorder:
    """the store as VisualPoseGraph sees it, with findConnection replaced by a note of what it was asked"""

    def __init__(self, store):
        self._store, self.asked = store, []

    def __getattr__(self, name):
        return getattr(self._store, name)

    def findConnection(self, cur, olds, qic, tic, params=None):
        self.asked.append((cur, list(olds)))
        return [dict(has_loop=False) for _ in olds]


def test_pose_graph_hands_the_detectors_candidate_to_find_connection(solver, voc10k, driven):
    from vil_fusion_amd.visual_posegraph import VisualPoseGraph
    voc, V = voc10k
    frames, db, want = driven
    loops = {i: r["loop_index"] for i, r in enumerate(want) if r["loop_index"] != -1}
    rec = Recorder(make(solver, voc))
    g = VisualPoseGraph(rec)
    for i, f in enumerate(frames):
        bc.load(rec, f)
        assert g.addKeyFrame(i, 0, np.eye(3), np.array([0.1 * i, 0.0, 0.0]), detect_loop=True) == -1      # the recorder verifies nothing
    assert rec.asked == [(i, [l]) for i, l in sorted(loops.items())] and len(loops) > 0
    # the default call: the caller's candidates as before, and the key frame goes into the database all the same
    rec2 = Recorder(make(solver, voc))
    g2 = VisualPoseGraph(rec2)
    for i, f in enumerate(frames[:6]):
        bc.load(rec2, f)
        g2.addKeyFrame(i, 0, np.eye(3), np.zeros(3), candidates=[0] if i == 4 else ())
    assert rec2.asked == [(4, [0])] and rec2.bow_size() == 6
    same_vector(rec2.bow_vector(5), db.entries[5])
    rec3 = Recorder(make(solver))                                                                  # no vocabulary: nothing changes
    g3 = VisualPoseGraph(rec3)
    bc.load(rec3, frames[0])
    assert g3.addKeyFrame(0, 0, np.eye(3), np.zeros(3)) == -1 and rec3.asked == [] and rec3.bow_size() == 0
