"""A Python restatement of the candidate loop of ScanContextClosure::SearchAndAddConstraint
(tbv_slam/src/tbv_slam/loopclosure.cpp:653-724) up to the registration, for the rows cfear_sc_detect_batch writes for a
batch of graphs: the row -> (from, to, guess_nr) mapping (:660-661, 675), the narrowing of the similarity to float (:677),
the speedup rule (:682-688), Tsrcguess = Taug^-1 * Rz(yaw) under transl_guess (:692-696), the query (the group
ApplyConstratins runs over, :724) and VerifyByOdometry (:776-806, from oracle.pyoracle).  What tests compare
cfear_verify_sc_rows against; no GPU, no library."""
import numpy as np

from oracle import pyoracle as O

SPEEDUP_ODOM = 0.7                      # loopclosure.cpp:683


def guess_of(taug, yaw, transl_guess=True):
    """Tsrcguess (:692-696): rot_offset = AngleAxis(-src_yaw_offset) = a rotation by sc_cand_yaw, a float widened to double."""
    rot = np.array([0.0, 0.0, float(np.float32(yaw))])
    if not transl_guess:
        return rot
    return O.xyt_compose(O.xyt_inverse(np.asarray(taug, np.float64)), rot)


def odom_bounds_of(rel_xyt, node0, frm, to, odom_sigma_error=0.03, verify_via_odometry=True):
    """VerifyByOdometry(from, to): RelativeMotion(i, i + 1) for i = to .. from - 1 of the graph that starts at flat node node0."""
    if not verify_via_odometry:
        return 1.0
    return O.verify_by_odometry(np.asarray(rel_xyt, np.float64).reshape(-1, 3)[node0 + to:node0 + frm], odom_sigma_error, True)


def rows_to_candidates(rows, n_out, node_off, n_detect=None, rel_xyt=None, transl_guess=True, speedup=False,
                       odometry_coupled_closure=True, odom_sigma_error=0.03, verify_via_odometry=True):
    """rows [D][n_candidates] records with min_dist, min_dist_odom, yaw_diff_rad, nn_idx, Taug; n_out [D]; node_off [G + 1];
    n_detect [G] (default: every node).  -> the compacted candidates in (row, guess_nr) order, one dict each:
    graph, from, to, guess_nr, query (the flat node index of from), skip, guess_xyt, sc_sim, odom_term, and odom_bounds
    (None for a skipped candidate: the reference never computes it there)."""
    node_off = np.asarray(node_off, np.int64)
    G = len(node_off) - 1
    nd = np.diff(node_off) if n_detect is None else np.asarray(n_detect, np.int64)
    first = np.concatenate([[0], np.cumsum(nd)])
    out = []
    for g in range(G):
        for d in range(int(first[g]), int(first[g + 1])):
            frm = d - int(first[g])
            for s in range(int(n_out[d])):                                  # records past n_out[d] are ignored
                r = rows[d][s]
                c = dict(graph=g, to=int(r["nn_idx"]), guess_nr=s, query=int(node_off[g]) + frm)
                c["from"] = frm
                skip = bool(odometry_coupled_closure and speedup and float(r["min_dist_odom"]) > SPEEDUP_ODOM)
                c["skip"] = int(skip)
                c["guess_xyt"] = guess_of(r["Taug"], r["yaw_diff_rad"], transl_guess)
                c["sc_sim"] = float(r["min_dist"]) if skip else float(np.float32(r["min_dist"]))     # :684 / :677
                c["odom_term"] = float(r["min_dist_odom"])
                c["odom_bounds"] = None if skip or rel_xyt is None and verify_via_odometry else odom_bounds_of(
                    rel_xyt, int(node_off[g]), frm, c["to"], odom_sigma_error, verify_via_odometry)
                out.append(c)
    return out


def skipped_record(c):
    """What a skipped candidate reports (UpdateStatistics at :684; the constraint is never registered): the fields of a
    cfear_verify_result that are not zero, `rank` as host results carry it."""
    return dict(reg_ok=0, t_be=np.zeros(3), cov=np.eye(6), coral=np.zeros(3), cfear=np.zeros(3), alignment_quality=-20.0,
                odom_bounds=c["odom_term"], sc_sim=c["sc_sim"], probability=0.0, accepted=0, rank=-1)
