#!/usr/bin/env python3
"""Candidate-retrieval replay timing: a seeded k = 10, L = 6 vocabulary (1 111 110 nodes, 10^6 words: the shape of the reference's brief_k10L6.bin) and N loaded key
frames (default 4096) of about 1000 descriptors, the second half of the drive revisiting the first, then
  add      vilf_kf_bow_add_range over all key frames (one bow_transform launch over all descriptors, one radix sort, one bow_compact launch)
  replay   vilf_kf_bow_detect_range over all key frames (bow_score and bow_select, in batches of at most 2^23 score cells)
  check    the first 64 key frames through tests/bow_reference.py (plain Python) and through the device, compared to the bit; the restatement's time on that slice is
           the only yardstick there is for a new stage: context, not a comparison of like with like
Stage times are HIP events under vilf_set_profiling (vilf_kf_bow_profile); wall times include the copies and the host side of the call. Every number is the best of
three repetitions after a warm-up of the same shape; all three are kept in the output.

  python tools/dev_bow_replay.py [--n 4096] [--desc 1000] [--out profiles/bow_replay.json]    # the steps as child processes, each under its own `timeout`, stops at the first that fails
  python tools/dev_bow_replay.py --step add|replay|check                                      # one step in this process; prints one JSON line"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np

STEP_TIMEOUT = {"add": 420, "replay": 420, "check": 600}
CAM = (460.0, 460.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)


def flip_masks(rng, n, bits):
    """(n, 4) uint64 masks with up to `bits` random bits set (positions drawn with replacement: a pair of equal draws cancels)"""
    m = np.zeros((n, 4), dtype=np.uint64)
    rows = np.arange(n)
    for _ in range(bits):
        pos = rng.integers(0, 256, size=n)
        m[rows, pos // 64] ^= np.uint64(1) << (pos % 64).astype(np.uint64)
    return m


def make_vocabulary(seed=1, k=10, L=6, flips=12):
    """tests/bow_cases.tree, level by level in numpy: ids in breadth-first order, a child = its parent with `flips` bits flipped, weights log(N / n_i)"""
    from vil_fusion_amd import abi
    rng = np.random.default_rng(seed)
    ids, parents, descs = [], [], []
    pid, pdesc, nxt = np.zeros(1, dtype=np.int64), None, 1
    for depth in range(1, L + 1):
        n = len(pid) * k
        d = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64) if pdesc is None else np.repeat(pdesc, k, axis=0) ^ flip_masks(rng, n, flips)
        i = np.arange(nxt, nxt + n)
        ids.append(i); parents.append(np.repeat(pid, k)); descs.append(d)
        pid, pdesc, nxt = i, d, nxt + n
    nodes = np.zeros(nxt - 1, dtype=abi.BOW_NODE_DTYPE)
    nodes["nodeId"], nodes["parentId"], nodes["descriptor"] = np.concatenate(ids), np.concatenate(parents), np.concatenate(descs)
    nodes["weight"] = np.log(1000.0 / rng.integers(1, 1000, size=len(nodes)))
    words = np.zeros(len(ids[-1]), dtype=abi.BOW_WORD_DTYPE)
    words["nodeId"], words["wordId"] = ids[-1], np.arange(len(ids[-1]))
    return dict(k=k, L=L, scoringType=0, weightingType=0, nodes=nodes, words=words), descs[-1]


def make_keyframes(leaves, n, n_desc, seed=2, noise=3):
    """n descriptor sets: a key frame keeps a third of its predecessor's words, key frame n / 2 + j keeps 70 % of key frame j's; every descriptor is a leaf with up
    to `noise` bits flipped"""
    rng = np.random.default_rng(seed)
    words = []
    for i in range(n):
        if i >= n // 2 and i - n // 2 < len(words):
            keep = rng.choice(words[i - n // 2], size=int(0.7 * n_desc), replace=False)
        elif i:
            keep = rng.choice(words[-1], size=n_desc // 3, replace=False)
        else:
            keep = np.zeros(0, dtype=np.int64)
        words.append(np.concatenate([keep, rng.integers(0, len(leaves), size=n_desc - len(keep))]))
    return [leaves[w] ^ flip_masks(rng, len(w), noise) for w in words]


def setup(n, n_desc):
    from vil_fusion_amd.estimator import BackendSolver, KeyFrameStore
    import kf_reference as kr
    t0 = time.perf_counter()
    voc, leaves = make_vocabulary()
    frames = make_keyframes(leaves, n, n_desc)
    s = BackendSolver()
    store = KeyFrameStore(s, 64, 48, CAM, kr.read_pattern(), cap_keyframes=n, cap_keypoints=n * n_desc)
    z, e2, e4 = np.zeros((n_desc, 2), dtype=np.float32), np.zeros((0, 2), dtype=np.float32), np.zeros((0, 4), dtype=np.uint64)
    for f in frames:
        store.add_loaded(z, z, f, e2, e4)
    store.set_vocabulary(voc)
    return s, store, voc, frames, time.perf_counter() - t0


def timed(s, store, call):
    s._check(s._L.vilf_set_profiling(s._h, 1), "vilf_set_profiling")
    t = time.perf_counter()
    res = call()
    wall = time.perf_counter() - t
    prof = store.bow_profile()
    s._check(s._L.vilf_set_profiling(s._h, 0), "vilf_set_profiling")
    return res, dict(wall_ms=1e3 * wall, **{k + "_ms": v[0] for k, v in prof.items() if v[1]}, **{k + "_spans": v[1] for k, v in prof.items() if v[1]})


def gpu_step(step, n, n_desc):
    s, store, voc, frames, setup_s = setup(n, n_desc)
    out = dict(step=step, n=n, descriptors=int(sum(len(f) for f in frames)), nodes=len(voc["nodes"]) + 1, words=len(voc["words"]), setup_s=setup_s)
    if step == "add":
        store.bow_add_range(0, n)                           # warm-up: allocations, code object load
        runs = []
        for _ in range(3):
            store.set_vocabulary(voc)                       # drops the database
            runs.append(timed(s, store, lambda: store.bow_add_range(0, n))[1])
        out.update(runs=runs, transform_ms=min(r["transform_ms"] for r in runs), sort_compact_ms=min(r["sort_compact_ms"] for r in runs))
        out["vector_words"] = int(sum(len(store.bow_vector(i)[0]) for i in range(0, n, max(n // 64, 1)))) // len(range(0, n, max(n // 64, 1)))
        out["descriptors_per_s"] = out["descriptors"] / (out["transform_ms"] * 1e-3)
    elif step == "replay":
        store.bow_add_range(0, n)
        store.detect_loop_range(0, n)                       # warm-up
        runs = []
        for _ in range(3):
            res, r = timed(s, store, lambda: store.detect_loop_range(0, n))
            runs.append(r)
        pairs = sum(q if q == 49 else max(q - 50, 0) + (q > 0) for q in range(n))      # eligible (query, entry) pairs: e < q - 50 and the newest; all at 49
        words = int(sum(len(store.bow_vector(i)[0]) for i in range(0, n, max(n // 64, 1)))) // len(range(0, n, max(n // 64, 1)))
        out.update(runs=runs, score_ms=min(r["score_ms"] for r in runs), select_ms=min(r["select_ms"] for r in runs), pairs=pairs, vector_words=words,
                   loops=sum(r["loop_index"] != -1 for r in res), loops_second_half=sum(r["loop_index"] != -1 for r in res[n // 2:]))
        out["entry_bytes_read"] = pairs * words * 12
        out["entry_GBps"] = out["entry_bytes_read"] / (out["score_ms"] * 1e-3) / 1e9
        # the batches of the replay against one piece that needs none: the same rows, to the bit
        tail = store.detect_loop_range(n - 64, 64)
        out["batched_equals_single"] = all(a["loop_index"] == b["loop_index"] and np.array_equal(a["id"], b["id"]) and
                                           np.array_equal(a["score"].view(np.uint64), b["score"].view(np.uint64)) for a, b in zip(res[n - 64:], tail))
        assert out["batched_equals_single"]
    else:
        import bow_reference as br
        m = min(64, n)
        store.bow_add_range(0, m)
        got = store.detect_loop_range(0, m)
        t = time.perf_counter()
        V = br.Vocabulary(voc)
        out["reference_vocabulary_s"] = time.perf_counter() - t
        db = br.Database(V)
        t = time.perf_counter()
        for f in frames[:m]:
            db.add(f)
        out["reference_add_s"] = time.perf_counter() - t
        t = time.perf_counter()
        want = db.detect_loop_range(0, m)
        out["reference_replay_s"] = time.perf_counter() - t
        same = all(g["loop_index"] == w["loop_index"] and np.array_equal(g["id"], w["id"]) and np.array_equal(g["score"].view(np.uint64), w["score"].view(np.uint64))
                   for g, w in zip(got, want))
        same = same and all(np.array_equal(store.bow_vector(i)[0], np.array(db.entries[i][0], dtype=np.int32)) and
                            np.array_equal(store.bow_vector(i)[1].view(np.uint64), np.array(db.entries[i][1]).view(np.uint64)) for i in range(m))
        out.update(slice=m, device_equals_reference=bool(same))
        assert same
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--desc", type=int, default=1000)
    ap.add_argument("--step", choices=list(STEP_TIMEOUT))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(gpu_step(a.step, a.n, a.desc)))
        return 0
    lines = []
    for step in STEP_TIMEOUT:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(a.n), "--desc", str(a.desc)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
