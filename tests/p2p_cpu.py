"""NumPy restatement of p2pQuality / keypointRepetability (coral_alignment_quality/src/alignment_checker/
AlignmentQuality.cpp:235-328) and of scanEvaluator (ScanEvaluator.cpp:4-114, ScanEvaluator.h:21-52).  It is the DEFINITION
cfear_p2p_quality_batch and api.scanEvaluator are compared against: every float operation is its own rounding, in the
reference's order (built for baseline x86-64: no FMA).

  Tchange = Tref.inverse() * Tsrc * Toffset       planar poses as (2x2 linear part, translation); the inverse is
                                                  (R^T, -R^T t); products are plain fp64, left to right
  moved point                                     pcl::transformPointCloud<PointXYZI, double>: float(((T0 x + T1 y) + 0 z) + T2)
  radiusSearch                                    3-D, d = (dx dx + dy dy) + dz dz in float, kept when d < float(r * r), strictly
  residuals_                                      {0, 0, 0} of the base constructor, then the nearest d per matched point

UNPINNED: Eigen's Affine3d::inverse() is a general 4x4-block inverse, so the reference's last bits of Tchange may differ from
the rigid-inverse formula here; cos / sin come from the host libm (math.cos), as in the library's host code."""
import math

import numpy as np

F = np.float32
HEADER = ["index", "ref_id", "src_id", "distance", " score1", "score2", "score3", "aligned", "error x", "error y", "error theta"]


def affine(xyt):
    """(x, y, theta) -> (l0, l1, l2, l3, t0, t1): [c -s; s c] and the translation."""
    c, s = math.cos(float(xyt[2])), math.sin(float(xyt[2]))
    return (c, -s, s, c, float(xyt[0]), float(xyt[1]))


def inverse(a):
    l0, l1, l2, l3, t0, t1 = a
    return (l0, l2, l1, l3, -(l0 * t0 + l2 * t1), -(l1 * t0 + l3 * t1))


def product(a, b):
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3],
            a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[0] * b[4] + a[1] * b[5] + a[4], a[2] * b[4] + a[3] * b[5] + a[5])


def tchange(ref_pose, src_pose, offset=(0.0, 0.0, 0.0)):
    """Tref.inverse() * Tsrc * Toffset as the job's T[6]: row-major 2x3."""
    m = product(product(inverse(affine(ref_pose)), affine(src_pose)), affine(offset))
    return np.array([m[0], m[1], m[4], m[2], m[3], m[5]], np.float64)


def transform(src, T):
    """float32 [n, 3]: the source points moved by T, z carried through."""
    src = np.asarray(src, F).reshape(-1, 4)
    x, y, z = (src[:, k].astype(np.float64) for k in range(3))
    out = np.empty((src.shape[0], 3), F)
    out[:, 0] = (((T[0] * x + T[1] * y) + 0.0 * z) + T[2]).astype(F)
    out[:, 1] = (((T[3] * x + T[4] * y) + 0.0 * z) + T[5]).astype(F)
    out[:, 2] = src[:, 2]
    return out


def nearest(ref, moved, radius, chunk=256):
    """float32 [n_src]: the smallest kept d of every moved point, -1 where none is kept."""
    ref = np.asarray(ref, F).reshape(-1, 4)
    r2 = F(float(radius) * float(radius))
    out = np.full(moved.shape[0], F(-1), F)
    if ref.shape[0] == 0:
        return out
    for s in range(0, moved.shape[0], chunk):
        q = moved[s:s + chunk]
        dx = q[:, None, 0] - ref[None, :, 0]
        dy = q[:, None, 1] - ref[None, :, 1]
        dz = q[:, None, 2] - ref[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F
        kept = d < r2
        best = np.where(kept, d, F(np.inf)).min(axis=1)
        out[s:s + chunk] = np.where(kept.any(axis=1), best, F(-1))
    return out


def p2p(ref, src, T, radius=3.0):
    """dict(per_point, matched, n_src, sum, mean, residuals, quality, repeatability) of one (ref, src, T, radius)."""
    src = np.asarray(src, F).reshape(-1, 4)
    per_point = nearest(ref, transform(src, np.asarray(T, np.float64)), radius)
    hit = per_point >= 0
    res = per_point[hit].astype(np.float64)
    total = 0.0
    for v in res:                                                   # the serial fp64 sum of GetQualityMeasure (:242-246)
        total += float(v)
    matched, n_src = int(hit.sum()), int(src.shape[0])
    mean = total / float(matched + 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = float(np.float64(matched) / np.float64(n_src))       # 0.0 / 0.0 = NaN for an empty source cloud
    return dict(per_point=per_point, matched=matched, n_src=n_src, sum=total, mean=mean,
                residuals=[0.0, 0.0, 0.0] + [float(v) for v in res], quality=[mean, 0.0, 0.0],
                repeatability=[rel, float(matched), float(n_src)])


def create_perturbations(offset_rotation_steps=2, theta_range=2 * math.pi / 4.0, range_error=0.5,
                         theta_error=0.57 * math.pi / 180.0):
    """scanEvaluator::CreatePerturbations (ScanEvaluator.cpp:11-25); the defaults are ScanEvaluator.h:63-78."""
    vek = [[0.0, 0.0, 0.0]]                                         # the aligned offset, then the ring of misaligned ones
    for i in range(offset_rotation_steps):
        angle = (float(i) / float(offset_rotation_steps)) * theta_range
        vek.append([range_error * math.cos(angle), range_error * math.sin(angle), theta_error])
    return vek


def aligned(perturbation):                                          # datapoint::aligned (:4-10)
    total = 0.0
    for e in perturbation:
        total += abs(e)
    return total < 0.0001


def evaluate(scans, method="P2P", radius=3.0, scan_spacing=1, **pert):
    """The pair loop of scanEvaluator (:65-109) over scans = [{"T": (x, y, theta), "cloud": float32 [n, 4][, "pose_id"]}].
    -> list of datapoints: dict(index, ref_id, src_id, distance, score, aligned, perturbation, residuals)."""
    vek = create_perturbations(**pert)
    out = []
    index = 0
    for k in range(scan_spacing, len(scans)):
        ref, src = scans[k - 1], scans[k]                           # prev_scans.back(), current
        index += 1
        for verr in vek:
            r = p2p(ref["cloud"], src["cloud"], tchange(ref["T"], src["T"], verr), radius)
            if method == "P2P":
                score, res = r["quality"], r["residuals"]
            elif method == "keypoint_repetability":
                score, res = r["repeatability"], [0.0, 0.0, 0.0]
            else:
                raise ValueError(method)
            dx, dy = float(ref["T"][0]) - float(src["T"][0]), float(ref["T"][1]) - float(src["T"][1])
            out.append(dict(index=index, ref_id=int(ref.get("pose_id", k - 1)), src_id=int(src.get("pose_id", k)),
                            distance=math.sqrt(dx * dx + dy * dy), score=list(score), aligned=aligned(verr),
                            perturbation=list(verr), residuals=res))
    return out


def vec2string(vec):                                                # Utils.cpp:596-604
    return ",".join(vec)


def vals_to_string(d):                                              # datapoint::ValsToString: std::to_string
    return ["%d" % d["index"], "%d" % d["ref_id"], "%d" % d["src_id"], "%f" % d["distance"], "%f" % d["score"][0],
            "%f" % d["score"][1], "%f" % d["score"][2], "%d" % int(d["aligned"]), "%f" % d["perturbation"][0],
            "%f" % d["perturbation"][1], "%f" % d["perturbation"][2]]


def eval_text(datapoints):
    """The text of eval.txt (scanEvaluator::SaveEvaluation, :41-44)."""
    return "".join(vec2string(v) + "\n" for v in [HEADER] + [vals_to_string(d) for d in datapoints])


def synthetic_sequence(n=8, seed=11, points=300, noise=0.03, scan_type="kstrongStructuredRadar"):
    """n scans of one random planar world seen from poses along a gentle arc, each with its own measurement noise: the
    aligned offset scores best under P2P (checked on the CPU in tests/test_p2p_cpu.py before the GPU test relies on it)."""
    rng = np.random.default_rng(seed)
    world = (rng.uniform(-25, 25, (points, 4)) * [1, 1, 0, 1]).astype(F)
    scans = []
    for k in range(n):
        T = (0.8 * k, 0.1 * k, 0.02 * k)
        c, s = math.cos(T[2]), math.sin(T[2])
        dx = world[:, 0] - T[0] + rng.normal(0, noise, points)
        dy = world[:, 1] - T[1] + rng.normal(0, noise, points)
        cloud = world.copy()
        cloud[:, 0], cloud[:, 1] = c * dx + s * dy, -s * dx + c * dy
        scans.append({"T": T, "cloud": np.ascontiguousarray(cloud, F), "pose_id": 100 + k, "type": scan_type})
    return scans
