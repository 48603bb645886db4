"""NumPy float64 restatement of cfear_logreg_fit_batch (csrc/logreg.hip): sklearn's binary logistic-regression objective

    F(w, b) = 1/2 w.w + C * sum_i s_i * [log(1 + exp(z_i)) - y_i z_i],   z_i = w.x_i + b,   y_i in {0, 1},
    s_i = n / (2 n_class(i)) with class_weight="balanced", else 1      (no penalty on the intercept)

minimised by a damped Newton iteration: full step from the Jacobi-scaled LDL^T solve of the (d + 1)^2 system, Armijo
backtracking (1e-4, halving), stop when the Newton decrement -g.dw is at most 1e-16 * max(1, |F|) or no trial step down
to 2^-20 decreases F.  F is strictly convex when both classes are present, so the minimiser is unique and any exact
solver lands on it; the kernels are compared against this file, and this file against the coefficients the reference
ships and against sklearn (tests/test_logreg_cpu.py)."""
import numpy as np

OK, ERR_INVALID_ARGUMENT, ERR_SOLVER = 0, -1, -5
DEC_TOL, ARMIJO, MIN_STEP = 1e-16, 1e-4, 2.0 ** -20


def weights(y, balanced=True):
    n = y.shape[0]
    if not balanced:
        return np.ones(n)
    pos = y == 1
    return np.where(pos, n / (2.0 * max(int(pos.sum()), 1)), n / (2.0 * max(int((~pos).sum()), 1)))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def objective(X, y, w, b, C=1.0, balanced=True):
    z = X @ w + b
    return 0.5 * float(w @ w) + C * float(np.sum(weights(y, balanced) * (softplus(z) - y * z)))


def gradient(X, y, w, b, C=1.0, balanced=True, fit_intercept=True, dtype=np.float64):
    """(d + 1) gradient of F, intercept last; dtype=np.longdouble recomputes it in extended precision.  Also returns the
    largest absolute term of its sums (the scale its rounding is measured against)."""
    Xl, yl, wl = X.astype(dtype), y.astype(dtype), np.asarray(w, dtype)
    z = Xl @ wl + dtype(b)
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    r = dtype(C) * weights(y, balanced).astype(dtype) * (p - yl)
    g = np.concatenate([Xl.T @ r + wl, [r.sum() if fit_intercept else dtype(0)]])
    scale = max(float(np.abs(Xl * r[:, None]).max()), float(np.abs(r).max()), float(np.abs(wl).max()))
    return g, scale


def ldlt_solve(H, rhs):
    """H x = rhs by LDL^T of D^-1/2 H D^-1/2 (Jacobi scaling); None when a pivot is not positive."""
    n = H.shape[0]
    sc = 1.0 / np.sqrt(np.diag(H))
    if not np.all(np.isfinite(sc)):
        return None
    A = H * sc[:, None] * sc[None, :]
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = A[j, j] - np.sum(L[j, :j] ** 2 * D[:j])
        if not D[j] > 0.0:
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])) / D[j]
    v = rhs * sc
    for i in range(n):
        v[i] -= L[i, :i] @ v[:i]
    v /= D
    for i in range(n - 1, -1, -1):
        v[i] -= L[i + 1:, i] @ v[i + 1:]
    return v * sc


def check_rows(X, y):
    """The per-job refusals: no rows, a value that is not finite, a label that is not 0 or 1, one class only."""
    if X.shape[0] == 0 or not np.isfinite(X).all() or not np.isin(y, (0.0, 1.0)).all():
        return ERR_INVALID_ARGUMENT
    n_pos = int((y == 1).sum())
    return ERR_INVALID_ARGUMENT if n_pos in (0, X.shape[0]) else OK


def fit(X, y, C=1.0, balanced=True, fit_intercept=True, max_iterations=100):
    """-> dict(coef, intercept, objective, grad_inf, iterations, status, n_used, n_pos, confusion, balanced_accuracy)."""
    X, y = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(y, np.float64)
    n, d = X.shape
    out = dict(coef=np.zeros(d), intercept=0.0, objective=0.0, grad_inf=0.0, iterations=0, status=check_rows(X, y), n_used=n,
               n_pos=int((y == 1).sum()), confusion=np.zeros(4, np.int64), balanced_accuracy=0.0)
    if out["status"] != OK:
        return out
    s = C * weights(y, balanced)
    A = np.hstack([X, np.full((n, 1), 1.0 if fit_intercept else 0.0)])
    R = np.eye(d + 1)
    R[d, d] = 0.0
    v = np.zeros(d + 1)

    def F(v):
        z = A @ v
        return 0.5 * float(v[:d] @ v[:d]) + float(np.sum(s * (softplus(z) - y * z)))

    it, status = 0, OK
    while True:
        z = A @ v
        p = sigmoid(z)
        e = np.exp(-np.abs(z))
        f0 = 0.5 * float(v[:d] @ v[:d]) + float(np.sum(s * (softplus(z) - y * z)))
        g = A.T @ (s * (p - y)) + R @ v
        H = (A * (s * e / (1.0 + e) ** 2)[:, None]).T @ A + R
        if not fit_intercept:
            H[d, d] = 1.0
        dw = ldlt_solve(H, -g) if np.isfinite(f0) and np.isfinite(H).all() else None
        if dw is None or not np.isfinite(dw).all():
            status = ERR_SOLVER
            break
        dec = -float(g @ dw)
        if not dec > DEC_TOL * max(1.0, abs(f0)):
            break
        if it >= max_iterations:
            status = ERR_SOLVER
            break
        t = 1.0
        while t >= MIN_STEP and not F(v + t * dw) <= f0 - ARMIJO * t * dec:
            t *= 0.5
        if t < MIN_STEP:
            break
        v = v + t * dw
        it += 1
    out.update(coef=v[:d].copy(), intercept=float(v[d]), objective=f0, grad_inf=float(np.abs(g).max()), iterations=it, status=status)
    out["confusion"], out["balanced_accuracy"] = confusion(X, y, out["coef"], out["intercept"])
    return out


def confusion(X, y, w, b):
    """(tn, fp, fn, tp) at z > 0 and sklearn's balanced_accuracy_score."""
    pred = (X @ w + b) > 0
    pos = y == 1
    c = np.array([np.sum(~pos & ~pred), np.sum(~pos & pred), np.sum(pos & ~pred), np.sum(pos & pred)], np.int64)
    return c, 0.5 * (c[3] / float(c[2] + c[3]) + c[0] / float(c[0] + c[1]))


def margin_rows(X, w, b, rel=1e-9):
    """Rows whose sign of z is within rounding: |z| <= rel * (1 + sum_j |w_j x_ij|)."""
    return np.abs(X @ w + b) <= rel * (1.0 + np.abs(X * w[None, :]).sum(1))


# ---- the synthetic sets the CPU and GPU tests share ---------------------------------------------------------------------
def synthetic(seed, n, d, kind="plain"):
    """kind: plain (well scaled, overlapping classes), separable (a margin: only the penalty bounds w), degenerate (two nearly
    equal columns and one of scale 200, like #residuals next to an overlap in [0, 1]), skewed (3 % positives)."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    w = rng.randn(d)
    z = X @ w + 0.3
    if kind == "separable":
        y = (z > 0).astype(np.float64)
        X += np.outer(np.where(y > 0, 0.2, -0.2), w / np.linalg.norm(w))
    elif kind == "skewed":
        y = (z + rng.logistic(size=n) > np.quantile(z, 0.97)).astype(np.float64)
    else:
        y = (z + rng.logistic(size=n) > 0).astype(np.float64)
    if kind == "degenerate":
        if d >= 2:
            X[:, 1] = X[:, 0] + 1e-3 * rng.randn(n)
        X[:, d - 1] = 200.0 + 60.0 * X[:, d - 1]
    for c in (0.0, 1.0):                                       # both classes present whatever the draw
        if not (y == c).any():
            y[int(c)] = c
    return X, y


def ragged_batch(n_models=256, seed=7):
    """d = 1..8, 50 to 20 000 rows, every eighth model separable, every eighth (offset 4) near-degenerate, every 16th skewed."""
    rng = np.random.RandomState(seed)
    sets = []
    for m in range(n_models):
        d = 1 + m % 8
        n = int(np.exp(rng.uniform(np.log(50), np.log(20000))))
        n = 50 if m == 0 else 20000 if m == 1 else n
        kind = "separable" if m % 8 == 2 else "degenerate" if m % 8 == 6 else "skewed" if m % 16 == 5 else "plain"
        sets.append(synthetic(1000 + m, n, d, kind))
    return sets
