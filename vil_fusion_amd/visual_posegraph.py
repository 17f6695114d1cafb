"""The pose graph of the visual loop closure on the host (≙ PoseGraph, pose_graph/pose_graph.h and pose_graph.cpp): the three stages chained.

  stage one and two   KeyFrameStore.findConnection (vilf_kf_find_connection): BRIEF matching, PnP-RANSAC, the loop decision -> loop_info
  stage three         BackendSolver.optimize4dof (vilf_pg4_optimize): the 4-DoF graph over the key frames from the earliest looped one on, and the drift

What stays here is the bookkeeping of PoseGraph::addKeyFrame (:44-213) and the write-back of optimize4DoF (:535-575): sequences, the shift of a sequence into the
world frame on its first loop into another sequence, the drift applied to every new key frame. The caller names the candidates, as in stage two, or lets the store's
detectLoop name one (addKeyFrame(detect_loop=True): the DBoW2 query, vilf_kf_bow_detect). optimize4DoF runs when it is called, not on a thread that wakes every 2 s. Saving and loading the graph is not served."""
import numpy as np

from . import synth
from .sequence import R2ypr, ypr2R


class VisualPoseGraph:
    def __init__(self, store, backend=None, qic=None, tic=None, loop_params=None):
        """store: a KeyFrameStore (anything with findConnection(cur, olds, qic, tic, params=) and, for point_3d, set_geometry); backend: anything with
        optimize4dof(vio_R, vio_T, sequence, fixed, loops, params=) — the store's BackendSolver if not given. qic, tic: the camera-IMU extrinsic of findConnection."""
        self.store = store
        self.backend = backend if backend is not None else store.s
        self.qic = np.eye(3) if qic is None else np.asarray(qic, dtype=np.float64).reshape(3, 3)
        self.tic = np.zeros(3) if tic is None else np.asarray(tic, dtype=np.float64).reshape(3)
        self.loop_params = loop_params
        self.keyframes = {}                  # index -> dict, in the order they were added (keyframelist)
        self.sequence_cnt = 0
        self.sequence_loop = [0]
        self.earliest_loop_index = -1
        self.w_r_vio, self.w_t_vio = np.eye(3), np.zeros(3)
        self.r_drift, self.t_drift, self.yaw_drift = np.eye(3), np.zeros(3), 0.0
        self.optimize_buf = []

    def addKeyFrame(self, index, sequence, vio_R, vio_T, candidates=(), time_stamp=0.0, point_3d=None, detect_loop=False):
        """:44-213 for the stored key frame `index` (the caller has added it to the store). candidates: the old key frames to verify, in the caller's order; among
        those whose findConnection reports has_loop the first is the loop (the reference has one candidate). point_3d, if given, is handed to the store with the
        pose as the VIO gave it (origin_vio_R, origin_vio_T). detect_loop (:59-69): with it set and no candidates given, the candidate is store.detectLoop(index)
        if that is not -1; with it unset the key frame still goes into the store's database if a vocabulary is set there (addKeyFrameIntoVoc) and `index` is the
        database's next entry. Returns the loop's old index, or -1."""
        if index in self.keyframes:
            raise ValueError(f"key frame {index} is in the graph already")
        sequence = int(sequence)
        R0, T0 = np.array(vio_R, dtype=np.float64).reshape(3, 3), np.array(vio_T, dtype=np.float64).reshape(3)
        if sequence != self.sequence_cnt:
            if sequence != self.sequence_cnt + 1:
                raise ValueError(f"sequence {sequence} after sequence {self.sequence_cnt}: sequences are numbered in order")
            self.sequence_cnt += 1
            self.sequence_loop.append(0)
            self.w_t_vio, self.w_r_vio = np.zeros(3), np.eye(3)
            self.t_drift, self.r_drift, self.yaw_drift = np.zeros(3), np.eye(3), 0.0
        if point_3d is not None:
            self.store.set_geometry(index, point_3d, R0, T0)
        kf = dict(index=index, sequence=sequence, time_stamp=float(time_stamp), has_loop=False, loop_index=-1, loop_info=None,
                  vio_T=self.w_r_vio @ T0 + self.w_t_vio, vio_R=self.w_r_vio @ R0)
        loop_index = -1
        old = [int(c) for c in candidates]
        if detect_loop and not old:
            found = self.store.detectLoop(index)
            old = [found] if found != -1 else []
        elif getattr(self.store, "has_vocabulary", False) and self.store.bow_size() == index:
            self.store.bow_add(index)
        if old:
            unknown = [c for c in old if c not in self.keyframes]
            if unknown:
                raise ValueError(f"candidates {unknown} are not in the graph")
            rows = self.store.findConnection(index, old, self.qic, self.tic, params=self.loop_params)
            hit = next((k for k, r in enumerate(rows) if r["has_loop"]), None)
            if hit is not None:
                loop_index = old[hit]
                r = rows[hit]
                kf.update(has_loop=True, loop_index=loop_index, loop_info=(np.array(r["relative_t"], dtype=np.float64), np.array(r["relative_q"], dtype=np.float64),
                                                                            float(r["relative_yaw"])))
                self._on_loop(kf, self.keyframes[loop_index])
        kf["T"] = self.r_drift @ kf["vio_T"] + self.t_drift
        kf["R"] = self.r_drift @ kf["vio_R"]
        self.keyframes[index] = kf
        return loop_index

    def _on_loop(self, cur, old):
        """:84-129"""
        if self.earliest_loop_index > old["index"] or self.earliest_loop_index == -1:
            self.earliest_loop_index = old["index"]
        rel_t, rel_q, _ = cur["loop_info"]
        w, x, y, z = rel_q
        w_P_cur = old["vio_R"] @ rel_t + old["vio_T"]
        w_R_cur = old["vio_R"] @ synth.q_to_R(np.array([x, y, z, w]))
        shift_yaw = R2ypr(w_R_cur)[0] - R2ypr(cur["vio_R"])[0]
        shift_r = ypr2R(np.array([shift_yaw, 0.0, 0.0]))
        shift_t = w_P_cur - w_R_cur @ cur["vio_R"].T @ cur["vio_T"]
        if old["sequence"] != cur["sequence"] and self.sequence_loop[cur["sequence"]] == 0:      # the whole sequence moves into the world frame
            self.w_r_vio, self.w_t_vio = shift_r, shift_t
            for kf in [cur] + [k for k in self.keyframes.values() if k["sequence"] == cur["sequence"]]:
                kf["vio_T"] = self.w_r_vio @ kf["vio_T"] + self.w_t_vio
                kf["vio_R"] = self.w_r_vio @ kf["vio_R"]
            self.sequence_loop[cur["sequence"]] = 1
        self.optimize_buf.append(cur["index"])

    def optimize4DoF(self, params=None):
        """:406-582, when called: the graph over the key frames from earliest_loop_index to the newest looped key frame, the poses written back, the new drift
        applied to the key frames after it. Returns the back-end's result dict (with "nodes": the indices optimised), or None if no loop has come in since the
        last call."""
        if not self.optimize_buf:
            return None
        cur_index, first = self.optimize_buf[-1], self.earliest_loop_index
        self.optimize_buf = []
        order = list(self.keyframes)
        nodes = [i for i in order[:order.index(cur_index) + 1] if i >= first]
        local = {i: k for k, i in enumerate(nodes)}
        kfs = [self.keyframes[i] for i in nodes]
        loops = []
        for k, kf in enumerate(kfs):
            if kf["has_loop"]:
                assert kf["loop_index"] >= first and kf["loop_index"] in local, (kf["index"], kf["loop_index"], first)
                loops.append((local[kf["loop_index"]], k, kf["loop_info"][0], kf["loop_info"][2]))
        out = self.backend.optimize4dof(np.array([kf["vio_R"] for kf in kfs]), np.array([kf["vio_T"] for kf in kfs]), [kf["sequence"] for kf in kfs],
                                        [1 if (kf["index"] == first or kf["sequence"] == 0) else 0 for kf in kfs], loops, params=params)
        for k, kf in enumerate(kfs):
            kf["T"], kf["R"] = np.array(out["t"][k], dtype=np.float64), np.array(out["R"][k], dtype=np.float64).reshape(3, 3)
        res = dict(out["result"])
        self.yaw_drift, self.r_drift, self.t_drift = float(res["yaw_drift"]), np.array(res["r_drift"]).reshape(3, 3), np.array(res["t_drift"]).reshape(3)
        for i in order[order.index(cur_index) + 1:]:
            kf = self.keyframes[i]
            kf["T"] = self.r_drift @ kf["vio_T"] + self.t_drift
            kf["R"] = self.r_drift @ kf["vio_R"]
        res["nodes"] = nodes
        res["history"] = out.get("history")
        return res

    def getPose(self, index):
        kf = self.keyframes[index]
        return kf["T"].copy(), kf["R"].copy()

    def getVioPose(self, index):
        kf = self.keyframes[index]
        return kf["vio_T"].copy(), kf["vio_R"].copy()

    def save_tum(self, path):
        """the key frames' poses in the format of :153-170: stamp with 9 digits, x y z qx qy qz qw with 5"""
        with open(path, "w") as f:
            for kf in self.keyframes.values():
                q = synth.R_to_q(kf["R"])
                f.write(f"{kf['time_stamp']:.9f} " + " ".join(f"{v:.5f}" for v in (*kf["T"], *q)) + "\n")
