"""The dense NumPy restatement of pose-graph optimisation that tests/test_pgo.py, tests/test_pgo_matrix_cpu.py and the GPU
tests hold cfear_pgo_solve and cfear_pgo_solve_batch to.  Plain fp64 NumPy; it shares no code with csrc/pgo_terms.hpp.

  DensePGO   the residual of PoseGraph3dErrorTerm (ceresoptimizer.h:62-97) for every odometry (type 0) and loop (type 1)
             constraint, all blocks at once: r = L [p_ab - p_meas; 2 vec(q_meas q_ab^-1)], L the lower Cholesky factor of
             the scaled information (the odom_* diagonal with replace_cov_by_identity, the constraint's own matrix without),
             loops scaled by 1 / loop_scaling and under CauchyLoss(loop_loss_limit); mini_loop / candidate constraints
             (types 2 and 3) are ignored.  The Jacobian is built per block: 12 tangent columns, for the block's two nodes,
             in closed form (jac="analytic") or by central differences through plus() (jac="numeric").
  dense_lm   the trust-region Levenberg-Marquardt of Ceres 2.1 with an EXACT dense solve of every step.  Returns
             (x, costs, history): history["iterations"] holds one record per iteration -- kind "accepted" / "rejected" /
             "invalid" and the decision margins it took -- history["exit"] is "max_iterations", "gradient", "radius",
             "parameter" or "function", and history["margins"] lists every (name, ratio) the run compared: a margin is the
             ratio of the two sides of a comparison, so 1 is the threshold itself."""
import numpy as np


def qmul(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(a):
    return np.asarray(a) * np.array([-1.0, -1.0, -1.0, 1.0])


def qrot(q, v):
    v = np.asarray(v)
    return qmul(qmul(q, np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], -1)), qconj(q))[..., :3]


def plus(pose, d):
    """EigenQuaternionParameterization::Plus on one pose [7] or on many [k, 7] with d [6] / [k, 6]."""
    pose = np.asarray(pose, float)
    d = np.broadcast_to(np.asarray(d, float), pose.shape[:-1] + (6,))
    out = pose.copy()
    out[..., :3] += d[..., :3]
    nd = np.linalg.norm(d[..., 3:], axis=-1)
    safe = np.where(nd > 0, nd, 1.0)
    dq = np.concatenate([(np.sin(nd) / safe)[..., None] * d[..., 3:], np.cos(nd)[..., None]], -1)
    out[..., 3:] = np.where((nd > 0)[..., None], qmul(dq, pose[..., 3:]), pose[..., 3:])
    return out


DEFAULT_PAR = dict(loop_scaling=500000.0, odom_vxx=0.01, odom_vyy=0.01, odom_vtt=0.001, replace_cov_by_identity=1,
                   loop_loss_limit=0.1)
_E3 = np.eye(3)


class DensePGO:
    def __init__(self, constraints, ids, par, jac="analytic"):
        par = dict(DEFAULT_PAR, **par)
        idx = {int(i): k for k, i in enumerate(ids)}
        a, b, meas, Lm, cauchy = [], [], [], [], []
        for typ in (0, 1):
            for c in constraints:
                if c["type"] != typ:
                    continue
                f = 1.0 / par["loop_scaling"] if typ == 1 else 1.0
                if par["replace_cov_by_identity"]:
                    I = np.diag([1 / par["odom_vxx"], 1 / par["odom_vyy"], 1, 1, 1, 1 / par["odom_vtt"]]) * f
                else:
                    I = np.asarray(c["information"], float).reshape(6, 6) * f
                a.append(idx[int(c["id_begin"])])
                b.append(idx[int(c["id_end"])])
                meas.append(np.asarray(c["t_be"], float))
                Lm.append(np.linalg.cholesky(I))
                cauchy.append(typ == 1)
        self.a, self.b = np.array(a, int), np.array(b, int)
        self.meas, self.Lm, self.cauchy = np.array(meas).reshape(-1, 7), np.array(Lm).reshape(-1, 6, 6), np.array(cauchy, bool)
        self.m = self.a.size
        self.cauchy_b = float(par["loop_loss_limit"]) ** 2
        self.jac = jac

    def plain(self, xa, xb):
        """The residuals before the loss, [m, 6], of blocks whose begin / end nodes sit at xa / xb [m, 7]."""
        qai = qconj(xa[:, 3:])
        dq = qmul(self.meas[:, 3:], qconj(qmul(qai, xb[:, 3:])))
        e = np.concatenate([qrot(qai, xb[:, :3] - xa[:, :3]) - self.meas[:, :3], 2.0 * dq[:, :3]], 1)
        return np.einsum("mij,mj->mi", self.Lm, e)

    def _loss(self, r):
        s = (r * r).sum(1)
        rho0 = np.where(self.cauchy, self.cauchy_b * np.log(1.0 + s / self.cauchy_b), s)      # ceres::CauchyLoss, as written there
        rho1 = np.where(self.cauchy, 1.0 / (1.0 + s / self.cauchy_b), 1.0)
        return rho0, rho1

    def residuals(self, x):
        r = self.plain(x[self.a], x[self.b])
        rho0, rho1 = self._loss(r)
        return 0.5 * rho0.sum(), (r * np.sqrt(rho1)[:, None]).reshape(-1)

    def block_jacobians(self, x):
        """[m, 6, 12]: the plain residuals' derivatives with respect to the tangent (3 + 3) of the begin node, then the end node."""
        xa, xb = x[self.a], x[self.b]
        Jb = np.zeros((self.m, 6, 12))
        if self.jac == "numeric":
            h = 1e-6
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Jb[:, :, k] = (self.plain(plus(xa, d), xb) - self.plain(plus(xa, -d), xb)) / (2 * h)
                Jb[:, :, 6 + k] = (self.plain(xa, plus(xb, d)) - self.plain(xa, plus(xb, -d))) / (2 * h)
            return Jb
        # q <- exp(d) q turns the node by 2 d in the world frame: R <- (I + 2 [d]x) R.  With v = p_b - p_a,
        #   e_p = R_a^T v - p_meas        d e_p / d p_b = R_a^T = -d e_p / d p_a,   d e_p / d d_a = 2 R_a^T [v]x
        #   e_q = 2 vec(q_meas q_b^-1 q_a) d e_q / d d_a = 2 M = -d e_q / d d_b,    M[:, k] = vec(q_meas q_b^-1 (e_k, 0) q_a)
        qai = qconj(xa[:, 3:])
        v = xb[:, :3] - xa[:, :3]
        left = qmul(self.meas[:, 3:], qconj(xb[:, 3:]))
        E = np.zeros((self.m, 6, 12))
        for k in range(3):
            ek = np.broadcast_to(_E3[k], v.shape)
            rt = qrot(qai, ek)
            E[:, :3, k], E[:, :3, 6 + k] = -rt, rt
            E[:, :3, 3 + k] = 2.0 * qrot(qai, np.cross(v, ek))
            mk = qmul(qmul(left, np.concatenate([ek, np.zeros((self.m, 1))], 1)), xa[:, 3:])[:, :3]
            E[:, 3:, 3 + k], E[:, 3:, 9 + k] = 2.0 * mk, -2.0 * mk
        return np.einsum("mij,mjk->mik", self.Lm, E)

    def evaluate(self, x, want_jac):
        cost, r = self.residuals(x)
        if not want_jac:
            return cost, r, None
        n = x.shape[0]
        # Ceres scales the plain Jacobian by sqrt(rho') (Corrector, alpha = 0); it does not differentiate sqrt(rho')
        _, rho1 = self._loss(self.plain(x[self.a], x[self.b]))
        Jb = self.block_jacobians(x) * np.sqrt(rho1)[:, None, None]
        J = np.zeros((6 * self.m, 6 * n))
        rows = np.arange(6 * self.m).reshape(self.m, 6)
        for side, node in ((0, self.a), (1, self.b)):
            cols = 6 * node[:, None] + np.arange(6)[None, :]
            np.add.at(J, (rows[:, :, None], cols[:, None, :]), Jb[:, :, 6 * side:6 * side + 6])
        return cost, r, J[:, 6:]                                          # the first node is constant


def _ratio(lhs, rhs):
    if rhs == 0:
        return 1.0 if lhs == 0 else np.inf
    return lhs / rhs


def dense_lm(prob, x0, max_iter=200):
    x = x0.copy()
    n = x.shape[0]
    radius, dec, reuse, diag = 1e4, 2.0, False, None
    x_cost, r, J = prob.evaluate(x, True)
    g = J.T @ r
    scaling = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    J = J * scaling
    x_norm = np.linalg.norm(x[1:])
    summ = dict(cost=x_cost, ok=True, gmax=np.abs(g).max() if g.size else 0.0, it=0)
    costs, invalid = [], 0
    hist = dict(iterations=[], exit=None, margins=[])

    def margin(name, lhs, rhs, rec=None):
        m = _ratio(lhs, rhs)
        hist["margins"].append((name, m))
        if rec is not None:
            rec[name] = m

    while True:
        costs.append(summ["cost"])
        if summ["it"] >= max_iter:
            hist["exit"] = "max_iterations"
            break
        if summ["ok"]:
            margin("gradient", summ["gmax"], 1e-10)
            if summ["gmax"] <= 1e-10:
                hist["exit"] = "gradient"
                break
        if radius <= 1e-32:
            hist["exit"] = "radius"
            break
        summ = dict(cost=0.0, ok=False, gmax=summ["gmax"], it=summ["it"] + 1)
        rec = dict(kind=None)
        hist["iterations"].append(rec)
        if not reuse:
            diag = np.clip((J * J).sum(0), 1e-6, 1e32)
        A = J.T @ J + np.diag(diag / radius)
        step = -np.linalg.solve(A, J.T @ r)
        reuse = True
        mr = J @ step
        mcc = -mr @ (r + mr / 2)
        if not (mcc > 0):
            rec["kind"] = "invalid"
            invalid += 1
            assert invalid < 5
            radius /= dec; dec *= 2
            summ.update(cost=x_cost)
            continue
        invalid = 0
        delta = np.concatenate([np.zeros(6), step * scaling]).reshape(n, 6)
        cand = plus(x, delta)
        cand[0] = x[0]
        cand_cost, _, _ = prob.evaluate(cand, False)
        margin("parameter", np.linalg.norm((x - cand)[1:]), 1e-8 * (x_norm + 1e-8), rec)
        if np.linalg.norm((x - cand)[1:]) <= 1e-8 * (x_norm + 1e-8):
            rec["kind"], hist["exit"] = "exit", "parameter"
            break
        margin("function", abs(x_cost - cand_cost), 1e-6 * x_cost, rec)
        if abs(x_cost - cand_cost) <= 1e-6 * x_cost:
            rec["kind"], hist["exit"] = "exit", "function"
            break
        rel = (x_cost - cand_cost) / mcc
        margin("decrease", rel, 1e-3, rec)
        if rel > 1e-3:
            rec["kind"] = "accepted"
            x = cand
            x_norm = np.linalg.norm(x[1:])
            x_cost, r, J = prob.evaluate(x, True)
            g = J.T @ r
            J = J * scaling
            summ.update(cost=x_cost, ok=True, gmax=np.abs(g).max())
            radius = min(1e16, radius / max(1 / 3, 1 - (2 * rel - 1) ** 3))
            dec, reuse = 2.0, False
        else:
            rec["kind"] = "rejected"
            summ.update(cost=cand_cost)
            radius /= dec; dec *= 2; reuse = True
    return x, costs, hist
