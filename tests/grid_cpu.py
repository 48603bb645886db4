"""NumPy restatement of the rule cfear_kstrong_rowkeys_derive applies, and the reference's CFEAR-3 grid search as a list of
configurations (shared by the grid tests; no GPU, no library call in the rule itself)."""
import math

import numpy as np


def u8(z_min):
    """uchar((int)z_min): radar_driver.cpp:58 float -> int, radar_filters.cpp:212 int -> uchar (256 -> 0, 0.9 -> 0)."""
    return int(z_min) & 0xFF


def derive_selection(sel_range, sel_intensity, sel_count, k_c, z_min_c):
    """The selection of (k_c, z_min_c) from the selection of a superset (k_sup >= k_c, u_sup <= u_c): per row the top k_c
    entries of the ascending list, restricted to intensity >= u_c.  Same layout as the input (padding -1 / 0)."""
    rows, k_sup = sel_range.shape
    u_c = u8(z_min_c)
    sr = np.full((rows, k_c), -1, np.int32)
    si = np.zeros((rows, k_c), np.uint8)
    sc = np.zeros(rows, np.int32)
    for r in range(rows):
        n = int(sel_count[r])
        keep = [j for j in range(n) if j >= n - k_c and int(sel_intensity[r, j]) >= u_c]
        sc[r] = len(keep)
        sr[r, :len(keep)] = sel_range[r, keep]
        si[r, :len(keep)] = sel_intensity[r, keep]
    return sr, si, sc


def derive_rowkeys(sel_range, sel_intensity, sel_count, k_c, z_min_c, range_res, min_distance):
    """The kernel's output for one class and image: keys uint32 [rows, 64] (0 beyond the count), counts int32 [rows]."""
    rows = sel_range.shape[0]
    min_bin = int(math.ceil(float(np.float32(min_distance)) / float(np.float32(range_res))))     # radar_filters.cpp:315
    sr, si, sc = derive_selection(sel_range, sel_intensity, sel_count, k_c, z_min_c)
    keys = np.zeros((rows, 64), np.uint32)
    cnt = np.zeros(rows, np.int32)
    for r in range(rows):
        kept = [(int(si[r, j]) << 24) | int(sr[r, j]) for j in range(int(sc[r])) if int(sr[r, j]) > min_bin]
        cnt[r] = len(kept)
        keys[r, :len(kept)] = kept
    return keys, cnt


def rows_of(kind, rows, cols, seed):
    """Test rows: uniform random bytes, five values around a threshold of 60, or one value."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    if kind == "five":
        return rng.choice(np.array([0, 59, 60, 61, 255], np.uint8), (rows, cols))
    return np.full((rows, cols), int(rng.choice([0, 60, 255])), np.uint8)


# launch/oxford/eval/params/grid_search/oxford_cfear-3, in the order of utils/worker's loops (last fastest)
GRID_CFEAR3 = dict(submap_scan_size=[4, 5, 6], res=[2.5, 2.75, 3.0], kstrong_k_strongest=[30, 40, 50], kstrong_z_min=[50.0, 60.0, 70.0],
                   reg_loss_limit=[0.1, 0.2, 0.3], reg_weight_opt=[0, 4])
