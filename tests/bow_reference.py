"""Candidate retrieval of the visual loop closure, restated in plain Python from the reference's sources (the paragraph "Visual loop closure, candidate retrieval"
of include/vilfusion.h is the same text): PoseGraph::detectLoop and addKeyFrameIntoVoc (pose_graph/pose_graph.cpp:307-404), TemplatedVocabulary::loadBin and
transform (ThirdParty/DBoW/TemplatedVocabulary.h), BowVector (BowVector.cpp), TemplatedDatabase::queryL1 (TemplatedDatabase.h). Python floats are IEEE doubles and
every sum below is an explicit loop, so the order of the additions is the reference's. It takes the arrays of the C ABI: a vocabulary is the dict that
estimator.load_vocabulary returns, descriptors are (n, 4) uint64 with bit i in word i // 64 at position i % 64 (boost::dynamic_bitset from the four blocks, :1541).
Not restated: the L2 and the other scorings, the direct index (use_di is false, pose_graph.cpp:41)."""
import math
import numpy as np

MAX_DEPTH, MAX_RESULTS, LDS_WORDS = 16, 16, 2048
L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
DEFAULTS = dict(max_results=4, min_gap=50, neighbour_score=0.05, loop_score=0.015)      # pose_graph.cpp:322, :351, :355, :376


class Unsupported(ValueError):
    pass


def as_int(desc4):
    """four uint64 words -> one 256-bit integer"""
    return int(desc4[0]) | int(desc4[1]) << 64 | int(desc4[2]) << 128 | int(desc4[3]) << 192


def distance(a, b):
    """F::distance of FBrief: the Hamming distance"""
    return bin(a ^ b).count("1")


class Vocabulary:
    def __init__(self, voc):
        """loadBin (:1509-1561) with the checks the C ABI states. Node ids are the caller's; children keep the order of the node array (:1538)."""
        nodes, words = voc["nodes"], voc["words"]
        nN, nW = len(nodes), len(words)
        if nN < 1 or nW < 1 or nW > nN:
            raise ValueError("nNodes / nWords")
        if not 0 <= int(voc["weightingType"]) <= 3 or not 0 <= int(voc["scoringType"]) <= 5:
            raise ValueError("weightingType / scoringType")
        if int(voc["scoringType"]) != L1_NORM:
            raise Unsupported("scoringType")
        self.weighting = int(voc["weightingType"])
        self.n_words = nW
        self.children = [[] for _ in range(nN + 1)]      # m_nodes[pid].children
        self.parent, self.weight, self.desc, self.word_id = [None] * (nN + 1), [0.0] * (nN + 1), [0] * (nN + 1), [-1] * (nN + 1)
        seen = [False] * (nN + 1)
        for r in nodes:
            nid = int(r["nodeId"])
            if not 1 <= nid <= nN or seen[nid]:
                raise ValueError("node ids are not a permutation of 1 .. nNodes")
            seen[nid] = True
            w = float(r["weight"])
            if not math.isfinite(w) or w < 0.0:
                raise ValueError("weight")
        for r in nodes:
            nid, pid = int(r["nodeId"]), int(r["parentId"])
            if not 0 <= pid <= nN or pid == nid:
                raise ValueError("a parent does not exist")
            self.parent[nid], self.weight[nid], self.desc[nid] = pid, float(r["weight"]), as_int(r["descriptor"])
            self.children[pid].append(nid)               # file order
        depth, reached, level = {0: 0}, 1, [0]
        while level:
            nxt = []
            for n in level:
                for c in self.children[n]:
                    depth[c] = depth[n] + 1
                    if depth[c] > MAX_DEPTH:
                        raise ValueError("deeper than VILF_BOW_MAX_DEPTH")
                    nxt.append(c)
                    reached += 1
            level = nxt
        if reached != nN + 1:
            raise ValueError("a node is not reachable from the root")
        self.depth = depth
        used = [False] * nW
        for r in words:
            nid, wid = int(r["nodeId"]), int(r["wordId"])
            if not 1 <= nid <= nN:
                raise ValueError("a word names a node that does not exist")
            if not 0 <= wid < nW or used[wid]:
                raise ValueError("word id out of range or used twice")
            if self.children[nid]:
                raise ValueError("a word on an inner node")
            if self.word_id[nid] != -1:
                raise ValueError("a leaf named by two words")
            used[wid], self.word_id[nid] = True, wid
        if any(not self.children[n] and self.word_id[n] == -1 for n in range(1, nN + 1)):
            raise ValueError("a leaf without a word")

    def transform(self, f):
        """:1217-1258 for one descriptor (a 256-bit integer) -> (word_id, weight)"""
        final_id = 0
        while True:
            nodes = self.children[final_id]               # :1234
            final_id = nodes[0]                           # :1235
            best_d = distance(f, self.desc[final_id])     # :1237
            for nid in nodes[1:]:                         # :1239
                d = distance(f, self.desc[nid])
                if d < best_d:                            # :1243, strict
                    best_d, final_id = d, nid
            if not self.children[final_id]:               # :1253 isLeaf
                break
        return self.word_id[final_id], self.weight[final_id]

    def transform_all(self, descs):
        d = np.asarray(descs, dtype=np.uint64).reshape(-1, 4)
        out = [self.transform(as_int(r)) for r in d]
        return np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64)

    def bow_vector(self, descs):
        """:1065-1121 over the descriptors in their order -> (word ids ascending, values), two lists"""
        v = {}
        for r in np.asarray(descs, dtype=np.uint64).reshape(-1, 4):
            wid, w = self.transform(as_int(r))
            if not w > 0:                                 # :1092, :1115 "not stopped"
                continue
            if self.weighting in (TF_IDF, TF):
                v[wid] = v[wid] + w if wid in v else w    # addWeight, BowVector.cpp:34-46
            elif wid not in v:
                v[wid] = w                                # addIfNotExist, :50-58
        ids = sorted(v)                                   # a std::map iterates in key order
        vals = [v[i] for i in ids]
        norm = 0.0                                        # normalize, :62-84 (L1: mustNormalize of L1Scoring)
        for x in vals:
            norm += math.fabs(x)
        if norm > 0.0:
            vals = [x / norm for x in vals]
        return ids, vals


def query_l1(entries, vec, max_results, max_id):
    """queryL1 (TemplatedDatabase.h:656-723): entries is the list of stored (ids, values) vectors, vec the query's -> [(entry id, Score)]"""
    n_entries = len(entries)
    ifile = {}                                            # the inverted file: word -> [(entry, value)] in ascending entry order
    for e, (ids, vals) in enumerate(entries):
        for wid, d in zip(ids, vals):
            ifile.setdefault(wid, []).append((e, d))
    pairs = {}
    for wid, q in zip(*vec):                              # :665, ascending word id
        for e, d in ifile.get(wid, ()):                   # :674
            if e < max_id or max_id == -1 or e == n_entries - 1:       # :679
                value = math.fabs(q - d) - math.fabs(q) - math.fabs(d)      # :681
                pairs[e] = pairs[e] + value if e in pairs else value          # :683-692
    ret = sorted(pairs.items(), key=lambda p: (p[1], p[0]))                   # :708; equal scores to the lower id: this project's choice
    if max_results > 0 and len(ret) > max_results:        # :712
        ret = ret[:max_results]
    return [(e, -s / 2.0) for e, s in ret]                # :722


def decide(ret, frame_index, params):
    """pose_graph.cpp:351-387 -> (find_loop, loop index)"""
    find_loop = False
    if len(ret) >= 1 and ret[0][1] > params["neighbour_score"]:              # :351
        for i in range(1, len(ret)):
            if ret[i][1] > params["loop_score"]:                              # :355
                find_loop = True
    if find_loop and frame_index > params["min_gap"]:                         # :376
        min_index = -1
        for i in range(len(ret)):
            if min_index == -1 or (ret[i][0] < min_index and ret[i][1] > params["loop_score"]):      # :381
                min_index = ret[i][0]
        return find_loop, min_index
    return find_loop, -1


class Database:
    """db of PoseGraph: entry e is key frame e"""

    def __init__(self, voc):
        self.voc = voc if isinstance(voc, Vocabulary) else Vocabulary(voc)
        self.entries = []

    def __len__(self):
        return len(self.entries)

    def add(self, descs):
        """addKeyFrameIntoVoc (:391-404)"""
        self.entries.append(self.voc.bow_vector(descs))

    def result(self, vec, ret, frame_index, params):
        find_loop, loop_index = decide(ret, frame_index, params)
        ids = [e for e, _ in ret] + [-1] * (MAX_RESULTS - len(ret))
        sc = [s for _, s in ret] + [0.0] * (MAX_RESULTS - len(ret))
        return dict(loop_index=loop_index, find_loop=find_loop, n_results=len(ret), n_words=len(vec[0]), id=np.array(ids, dtype=np.int32), score=np.array(sc, dtype=np.float64), ret=ret)

    def detect_loop(self, descs, frame_index, **over):
        """detectLoop (:307-389): query, then add, then the decision. frame_index must be the number of entries (the C ABI's constraint)."""
        params = dict(DEFAULTS, **over)
        assert frame_index == len(self.entries)
        vec = self.voc.bow_vector(descs)
        ret = query_l1(self.entries, vec, params["max_results"], frame_index - params["min_gap"])      # :322
        self.entries.append(vec)                                                                       # :327
        return self.result(vec, ret, frame_index, params)

    def detect_loop_range(self, first, n, **over):
        """the replay over a database that holds the key frames already: query i sees the first + i entries before it"""
        params = dict(DEFAULTS, **over)
        out = []
        for f in range(first, first + n):
            vec = self.entries[f]
            out.append(self.result(vec, query_l1(self.entries[:f], vec, params["max_results"], f - params["min_gap"]), f, params))
        return out
