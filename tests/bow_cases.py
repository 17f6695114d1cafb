"""Seeded vocabularies and key frames for the candidate-retrieval tests (tests/test_bow_reference.py, tests/test_bow.py, tools/dev_bow_replay.py). A vocabulary is the
dict estimator.load_vocabulary returns. A child's descriptor is its parent's with a few random bits flipped, so a descriptor a few bits off a leaf lands on that leaf
and a revisited place scores as a revisit does; weights are log(N / n_i) of seeded document counts, as DBoW2's IDF."""
import math
import struct
import numpy as np
from vil_fusion_amd import abi


def rand_desc(rng, n=None):
    return rng.integers(0, 1 << 64, size=(4,) if n is None else (n, 4), dtype=np.uint64)


def flip(rng, desc, bits):
    """desc (4,) uint64 with `bits` distinct random bits flipped"""
    d = np.array(desc, dtype=np.uint64).copy()
    for b in rng.choice(256, size=int(bits), replace=False):
        d[b // 64] ^= np.uint64(1) << np.uint64(b % 64)
    return d


def idf_weight(rng, n_docs=1000):
    """log(N / n_i), n_i in 1 .. N - 1: positive"""
    return math.log(n_docs / float(rng.integers(1, n_docs)))


def assemble(records, weighting=abi.VILF_BOW_TF_IDF, scoring=abi.VILF_BOW_L1_NORM, k=10, L=3, words=None):
    """records: [(nodeId, parentId, weight, descriptor (4,))] in file order. words: [(nodeId, wordId)], or None: the leaves in ascending node id get 0, 1, ..."""
    nodes = np.zeros(len(records), dtype=abi.BOW_NODE_DTYPE)
    for i, (nid, pid, w, d) in enumerate(records):
        nodes[i] = (nid, pid, w, np.asarray(d, dtype=np.uint64))
    if words is None:
        parents = {int(p) for p in nodes["parentId"]}
        leaves = sorted(int(n) for n in nodes["nodeId"] if int(n) not in parents)
        words = [(n, i) for i, n in enumerate(leaves)]
    wa = np.zeros(len(words), dtype=abi.BOW_WORD_DTYPE)
    for i, (nid, wid) in enumerate(words):
        wa[i] = (nid, wid)
    return dict(k=k, L=L, scoringType=scoring, weightingType=weighting, nodes=nodes, words=wa)


def tree(seed, k=10, L=3, flips=16, weighting=abi.VILF_BOW_TF_IDF, stop_fraction=0.0, shuffle=False):
    """a full k-ary tree of depth L, ids 1 .. in breadth-first order (the reference file's shape). stop_fraction of the leaves get weight 0. shuffle: the node array
    in a seeded random order, so that the order of a node's children is not the order of their ids."""
    rng = np.random.default_rng(seed)
    records, level, nid = [], [(0, None)], 0
    for depth in range(1, L + 1):
        nxt = []
        for pid, pdesc in level:
            for _ in range(k):
                nid += 1
                d = rand_desc(rng) if pdesc is None else flip(rng, pdesc, flips)
                w = idf_weight(rng)
                if depth == L and rng.random() < stop_fraction:
                    w = 0.0
                records.append((nid, pid, w, d))
                nxt.append((nid, d))
        level = nxt
    if shuffle:
        records = [records[i] for i in rng.permutation(len(records))]
    return assemble(records, weighting=weighting, k=k, L=L)


def leaf_descriptors(voc):
    """(n_words, 4) uint64: row w is the descriptor of word w's leaf"""
    by_id = {int(r["nodeId"]): r["descriptor"] for r in voc["nodes"]}
    out = np.zeros((len(voc["words"]), 4), dtype=np.uint64)
    for r in voc["words"]:
        out[int(r["wordId"])] = by_id[int(r["nodeId"])]
    return out


def keyframe(rng, leaves, n, noise=3, words=None):
    """n descriptors: seeded leaves (or the leaves of `words`, in that order) with up to `noise` bits flipped each"""
    pick = rng.integers(0, len(leaves), size=n) if words is None else np.asarray(words)
    return np.array([flip(rng, leaves[w], rng.integers(0, noise + 1)) for w in pick], dtype=np.uint64).reshape(-1, 4)


def drive(seed, voc, n_kf=120, n_desc=100, revisit_from=100, revisit_to=10, noise=4, keep=(0.9, 0.02), n_leaves=None):
    """a drive of n_kf key frames (descriptor sets): key frame revisit_from + j sees the place of key frame revisit_to + j again, keeping a fraction of its
    descriptors that alternates between the two values of `keep` (so some revisits clear the thresholds and some do not), each with up to `noise` bits flipped, the
    rest new. Neighbours share a third of their descriptors, as consecutive key frames do. n_leaves: only the first so many words are drawn from."""
    rng = np.random.default_rng(seed)
    leaves = leaf_descriptors(voc)[:n_leaves]
    frames = []
    for i in range(n_kf):
        if i >= revisit_from:
            old = frames[revisit_to + (i - revisit_from)]
            m = int(round(keep[(i - revisit_from) % 2] * len(old)))
            kept = np.array([flip(rng, old[j], rng.integers(0, noise + 1)) for j in rng.choice(len(old), size=m, replace=False)], dtype=np.uint64).reshape(-1, 4)
            fresh = keyframe(rng, leaves, n_desc - m)
            frames.append(np.concatenate([kept, fresh]))
        elif i > 0:
            prev = frames[-1]
            m = n_desc // 3
            kept = np.array([flip(rng, prev[j], rng.integers(0, noise + 1)) for j in rng.choice(len(prev), size=m, replace=False)], dtype=np.uint64).reshape(-1, 4)
            frames.append(np.concatenate([kept, keyframe(rng, leaves, n_desc - m)]))
        else:
            frames.append(keyframe(rng, leaves, n_desc))
    return frames


def vocabulary_bytes(voc):
    """the VINS binary file of a vocabulary, field by field (ThirdParty/VocabularyBinary.hpp): six int32, the node records of 48 bytes, the word records of 8"""
    out = [struct.pack("<6i", voc["k"], voc["L"], voc["scoringType"], voc["weightingType"], len(voc["nodes"]), len(voc["words"]))]
    for r in voc["nodes"]:
        out.append(struct.pack("<iid4Q", int(r["nodeId"]), int(r["parentId"]), float(r["weight"]), *(int(x) for x in r["descriptor"])))
    for r in voc["words"]:
        out.append(struct.pack("<ii", int(r["nodeId"]), int(r["wordId"])))
    return b"".join(out)


def load(store, descs):
    """a descriptor set as a loaded key frame (vilf_kf_add_loaded): the key points' positions play no part in candidate retrieval"""
    d = np.ascontiguousarray(descs, dtype=np.uint64).reshape(-1, 4)
    z = np.zeros((len(d), 2), dtype=np.float32)
    return store.add_loaded(z, z, d, np.zeros((0, 2), dtype=np.float32), np.zeros((0, 4), dtype=np.uint64))
