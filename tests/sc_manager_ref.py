"""RSCManager restated on top of the CPU oracle (RadarScancontext.cpp:133-345), written independently of api.py and of the
library's C++: the recent-node exclusion, the odometry likelihood, OdometryNNSearch / VanillaKDNNSearch (with the tree
rebuilt on every 50th call) and detectLoopClosureID's ranking, for any geometry, K, candidate count, sigma, search ratio,
mode and augmentation.  Descriptors and distances come from the oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def ref_key_tree():
    """The reference's nanoflann ring-key tree (tests/test_ref_nanoflann.py), or None when oracle/_ref was not built."""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import test_ref_nanoflann as T
    if not os.path.exists(T.SO):
        return None
    L = T._ref()
    return lambda keys: T.RefKeyTree(L, keys)


def local_maps(clouds, poses, n_aggregate, ids=None):
    """ScansToLocalMap of every node, merged on the host (tests/test_gpu_sc_sequence.py _merge)."""
    from tests.test_gpu_sc_sequence import _merge
    ids = np.arange(len(clouds)) if ids is None else ids
    return [_merge(clouds, poses, ids, i, n_aggregate) for i in range(len(clouds))]


def _l2norm(qk, keys, sim10):
    """L2norm (:250-257) of the query key (+ a 0) against every key (+ 10 x its odometry similarity): a float accumulator,
    float differences promoted to double; vectorised over the database, sequential over the elements."""
    l2 = np.zeros(keys.shape[0], np.float32)
    for r in range(keys.shape[1]):
        e = (qk[r] - keys[:, r]).astype(np.float64)
        l2 = (l2.astype(np.float64) + e * e).astype(np.float32)
    e = (np.float32(0) - sim10).astype(np.float64)
    return (l2.astype(np.float64) + e * e).astype(np.float32)


def _l2_adaptor(keys, qk):
    """nanoflann::L2_Adaptor::evalMetric in float: groups of four squared differences summed first, then the tail."""
    e2 = (keys - qk[None]) ** 2
    d = np.zeros(keys.shape[0], np.float32)
    for c in range(0, e2.shape[1] - 3, 4):
        d = d + (((e2[:, c] + e2[:, c + 1]) + e2[:, c + 2]) + e2[:, c + 3])
    for c in range(e2.shape[1] // 4 * 4, e2.shape[1]):
        d = d + e2[:, c]
    return d


def reference_manager_run(maps, poses, odometry=True, augment=True, num_ring=40, num_sector=120, max_radius=80.0,
                          search_ratio=0.1, k_tree=10, n_candidates=3, sigma=0.05, tree="ref"):
    """maps: the local map of every node (in its frame), poses (x, y, theta).  -> per node the candidate list
    [(min_dist, min_dist_sc, nn_idx, argmin_shift, augmentation)], closest first.  tree = "ref": the vanilla search asks
    the reference's own nanoflann tree when oracle/_ref is built; "linear": a linear scan with the tree's metric, equal
    distances in index order (the library's documented tie order)."""
    from oracle import pyoracle as O
    R, S = num_ring, num_sector
    descs, keys, P, out = [], np.zeros((0, R), np.float32), [], []
    state = {"counter": 0, "n": 0, "ref": None}
    make_tree = ref_key_tree() if tree == "ref" else None
    shifts = [0.0] + ([-2.0, 2.0, -4.0, 4.0] if augment else [])
    for cloud, T in zip(maps, poses):
        cur = [O.sc_descriptor(cloud, R, S, max_radius, "sum", 1000.0, 0.0, dy) for dy in shifts]
        descs.append(cur[0])
        keys = np.concatenate([keys, O.sc_keys(cur[0])[0].astype(np.float32)[None]])
        P.append(np.asarray(T, float))
        if len(P) <= 2:
            n_ex = 2
        else:
            dsum, n_ex, prev, i = 0.0, 0, P[-1], len(P) - 1
            while i >= 0 and dsum < 10.0:
                dsum += np.linalg.norm(P[i][:2] - prev[:2]); prev = P[i]; n_ex += 1; i -= 1
        cur_i = len(P) - 1
        sim = np.zeros(cur_i)
        tprev, trav = P[-1][:2], 0.0
        for i in range(cur_i - 1, -1, -1):
            trav += np.linalg.norm(tprev - P[i][:2]); tprev = P[i][:2]
            err = max(np.linalg.norm(P[-1][:2] - P[i][:2]) - 5.0, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.float64(err) / np.float64(trav)
            sim[i] = 1.0 - np.exp(-rel * rel / (2 * sigma * sigma))
        if len(keys) < n_ex + 1:
            out.append([]); continue
        cands = []
        for k, d in enumerate(cur):
            qk = O.sc_keys(d)[0].astype(np.float32)
            if odometry:
                L = max(cur_i - 1 - n_ex, 0)
                l2 = _l2norm(qk, keys[:L], (10 * sim[:L]).astype(np.float32))
                idxs = [int(i) for i in np.argsort(l2, kind="stable")[:k_tree]]
            else:
                # VanillaKDNNSearch (:225-248): the tree is rebuilt on every 50th CALL only, from the keys older than the
                # recent-node exclusion at that moment; the zero-initialised index vector is copied whole
                if state["counter"] % 50 == 0:
                    state["n"] = max(len(keys) - n_ex, 0)
                    state["ref"] = make_tree(keys[:state["n"]].copy()) if (make_tree and state["n"] > 0) else None
                state["counter"] += 1
                idxs = [0] * k_tree
                if state["ref"] is not None:
                    nfound, ridx, _ = state["ref"].knn(qk, k_tree)
                    idxs[:nfound] = [int(i) for i in ridx[:nfound]]
                elif state["n"] > 0:
                    order = np.argsort(_l2_adaptor(keys[:state["n"]], qk), kind="stable")[:k_tree]
                    idxs[:len(order)] = [int(i) for i in order]
            for i in idxs:
                dsc, sh = O.sc_distance(d, descs[i], search_ratio)
                cands.append((dsc + sim[i] if odometry else dsc, dsc, i, sh, k))
                cands.sort(key=lambda c: c[0])
                cands = cands[:n_candidates]
        out.append(cands)
    return out
