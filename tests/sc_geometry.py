"""Scan Context test geometries and the helpers the geometry tests share: the distance kernel's LDS layout (which decides
its shift chunk and the shapes the library accepts), a NumPy restatement of the kernel's polar binning (to find the points
whose sector depends on how atan rounds), and the clouds the tests describe."""
import numpy as np

# (num_ring, num_sector, max_radius).  TBV's default; ring counts that leave a tail of the four-wide ring-key metric; a
# single ring / a single sector; the 5120-cell capacity; long sector axes, up to the largest the distance kernel accepts
# with one ring at the default search ratio (S_MAX, checked against the layout in test_oracle_scancontext.py).
S_MAX = 2543
GEOMETRIES = [(40, 120, 80.0), (37, 113, 80.0), (20, 60, 50.0), (64, 80, 120.0), (1, 8, 80.0), (8, 1, 80.0),
              (40, 128, 80.0), (1, 2048, 80.0), (1, S_MAX, 80.0)]
RATIOS = (0.0, 0.05, 0.1, 0.5, 1.0, 1.5, 2.5)

LDS_BYTES = 160 * 1024                 # what sc_distance_kernel may use (scancontext.hip kScDistLds)


def search_space_size(S, ratio):
    """m = 2 round(0.5 ratio S) + 1 shifts (std::round: half away from zero); a negative radius leaves one."""
    x = 0.5 * ratio * S
    rad = np.floor(abs(x) + 0.5) * np.sign(x)
    return 1 if rad < 0 else 2 * int(rad) + 1


def distance_layout(R, S, ratio):
    """sc_distance_layout: (bytes before the similarity matrix, chunk of shifts evaluated together, accepted)."""
    m = search_space_size(S, ratio)
    base = ((2 * R * S + 5 * S) * 8 + (2 + m) * 4 + 15) & ~15
    room = max(LDS_BYTES - base, 0) // (S * 8)
    chunk = max(1, min(room, m, 256, S))
    return base, chunk, base + S * 8 <= LDS_BYTES


def ratio_for_m(S, m):
    """A search_ratio whose search space has exactly m (odd) shifts."""
    r = (m - 1) / S                                   # 0.5 r S = (m - 1) / 2, an integer
    assert search_space_size(S, r) == m
    return r


def kernel_bins(xyzi, R, S, rmax, shift_y=0.0):
    """sc_acc_point's binning in NumPy with the correctly rounded float arctangent (as the GPU takes it):
    (ring [n], sector [n]), -1 for a dropped point."""
    c = np.asarray(xyzi, np.float32)
    x, y, z = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64), c[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if shift_y != 0.0:
            px = (((1.0 * x + 0.0 * y) + 0.0 * z) + 0.0).astype(np.float32)
            py = (((0.0 * x + 1.0 * y) + 0.0 * z) + shift_y).astype(np.float32)
        else:
            px, py = c[:, 0].copy(), c[:, 1].copy()
        rng_ = np.sqrt(px * px + py * py)                        # float32 throughout
        k = 180 / np.pi

        def at(v):
            return np.arctan(v.astype(np.float64)).astype(np.float32).astype(np.float64)
        th = np.zeros(len(c), np.float64)
        q1, q2 = (px >= 0) & (py >= 0), (px < 0) & (py >= 0)
        q3, q4 = (px < 0) & (py < 0), (px >= 0) & (py < 0)
        th[q1] = k * at(py[q1] / px[q1])
        th[q2] = 180 - k * at(py[q2] / -px[q2])
        th[q3] = 180 + k * at(py[q3] / px[q3])
        th[q4] = 360 - k * at(-py[q4] / px[q4])
        th = th.astype(np.float32).astype(np.float64)
        rr = np.ceil((rng_.astype(np.float64) / rmax) * R)
        ss = np.ceil((th / 360.0) * S)
        ring = np.clip(np.where(np.isnan(rr), 1, np.nan_to_num(rr, posinf=R, neginf=1)), 1, R).astype(int) - 1
        sec = np.clip(np.where(np.isnan(ss), 1, np.nan_to_num(ss, posinf=S, neginf=1)), 1, S).astype(int) - 1
        drop = rng_.astype(np.float64) > rmax
    ring[drop] = -1
    sec[drop] = -1
    return ring, sec


def ambiguous(xyzi, R, S, rmax, shift_y=0.0):
    """Points the CPU oracle (the C library's float atan) bins into another cell than the correctly rounded one."""
    from oracle import pyoracle as O
    orr, osc = O.sc_bins(xyzi, R, S, rmax, shift_y)
    kr, ks = kernel_bins(xyzi, R, S, rmax, shift_y)
    return (orr != kr) | (osc != ks)


def random_cloud(seed, R, S, rmax, n=2500):
    """Points over the whole disc and a little past its rim, integer intensities 0 .. 255; a few bins hit many times."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), np.float32)
    r = rng.uniform(0.0, 1.08 * rmax, n)
    a = rng.uniform(-np.pi, np.pi, n)
    c[:, 0], c[:, 1] = r * np.cos(a), r * np.sin(a)
    c[:, 2] = rng.normal(0.0, 1.0, n)
    c[:, 3] = rng.integers(0, 256, n)
    c[-200:, :2] = c[:8, :2][rng.integers(0, 8, 200)]           # stacked points
    return c


def edge_cloud(R, S, rmax):
    """Points every implementation must bin the same way: the origin, both axes with +0.0 and -0.0, ring edges
    k rmax / R, the rim (kept) and the next float past it (dropped), the diagonals (sector edges where 8 | S), and
    non-finite coordinates.  Intensity 1 + index, so every point is visible in a "sum" descriptor."""
    f = np.float32
    rim = f(rmax)
    past = np.nextafter(rim, f(np.inf))
    pts = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)]
    for v in (f(3.0), f(rmax / 2), rim):
        pts += [(v, 0.0), (v, -0.0), (-v, 0.0), (-v, -0.0), (0.0, v), (-0.0, v), (0.0, -v), (-0.0, -v)]
        pts += [(v / 2, v / 2), (-v / 2, v / 2), (-v / 2, -v / 2), (v / 2, -v / 2)]
    for k in range(1, R + 1):
        e = f(k * rmax / R)
        pts += [(e, 0.0), (0.0, e), (-e, 0.0), (0.0, -e), (np.nextafter(e, f(0)), 0.0), (np.nextafter(e, f(np.inf)), 0.0)]
    pts += [(past, 0.0), (0.0, past), (-past, 0.0), (0.0, -past)]
    inf, nan = np.inf, np.nan
    pts += [(nan, 0.0), (0.0, nan), (nan, nan), (inf, 0.0), (-inf, 0.0), (0.0, inf), (0.0, -inf), (inf, inf), (nan, 5.0),
            (-5.0, nan), (inf, nan)]
    c = np.zeros((len(pts), 4), np.float32)
    c[:, :2] = np.array(pts, np.float32)
    c[:, 3] = 1 + np.arange(len(pts))
    return c
