"""CPU: which k-strongest row-sweep kernel a call launches and which selection path each row takes.  cfear_kstrong_plan is
the launcher's own selection (host code, no device): every case of tests/kstrong_cases.py reaches the instantiation it
names, all 16 have a case, and the plan's invariants hold over a sweep of widths, alignments and thresholds.  The model of
kstrong_row's branches (kstrong_cases.row_path) takes the path every row is labelled with and keeps exactly the oracle's
keys, on every row of every case and on a seeded random sweep -- so the reach table printed under -s speaks for the kernel."""
import collections
import functools

import numpy as np
import pytest

from tests import kstrong_cases as K


@functools.lru_cache(maxsize=None)
def _images(name):
    return K.images(K.CASES[name])


def _oracle_keys(img, k, z_min):
    from oracle import pyoracle as O
    sr, si, sc = O.kstrongest(img, k, z_min)
    return [((si[r, :sc[r]].astype(np.uint32) << 24) | sr[r, :sc[r]].astype(np.uint32)) for r in range(img.shape[0])]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_reaches_the_instantiation_it_names(name):
    case = K.CASES[name]
    nchunk, vec, mask = case.inst
    p = K.plan(case)
    assert p["refused"] is None
    assert (p["nchunk"], p["vec"], p["mask"]) == case.inst and p["table_index"] == K.table_index(*case.inst), (name, p)
    assert nchunk == min(n for n in K.NCHUNKS if n * 1024 >= case.cols)
    assert p["u_zmin"] == K.u_zmin(case.z_min) and p["thi"] == int(p["u_zmin"] >= 128) and mask == int(p["u_zmin"] == 0)
    assert p["kpad"] == max((case.k + 3) // 4 * 4, 64)
    assert p["min_range_bin"] == int(np.ceil(np.float64(np.float32(case.min_distance)) / np.float64(np.float32(K.RANGE_RES))))
    # any address with the same low bits selects the same kernel; vec needs the address and the strides to be multiples of 4
    assert K.plan(case, base=case.offset + 0x7f00a000)["table_index"] == p["table_index"]
    strides_allow = case.stride % 4 == 0 and (case.batch == 1 or case.batch_stride % 4 == 0)
    assert [K.plan(case, base=a)["vec"] for a in range(4)] == [int(strides_allow), 0, 0, 0]
    # the image: 5 to 15 rows, no multiple of 4; candidates in the last 16-byte piece of the first and of the last row
    img = _images(name)
    uz = K.u_zmin(case.z_min)
    assert img.shape == (case.batch, case.rows, case.cols) and 5 <= case.rows <= 15 and case.rows % 4
    last_piece = (case.cols - 1) // 16 * 16
    for b in range(case.batch):
        assert (img[b, 0, last_piece:] >= uz).any() and (img[b, -1, last_piece:] >= uz).any(), (name, b)
    np.testing.assert_array_equal(img, K.images(case))          # the same every time
    buf, view = K.buffer(case, img)
    np.testing.assert_array_equal(view, img)
    inside = np.zeros(buf.size, bool)
    np.lib.stride_tricks.as_strided(inside[case.offset:], view.shape, view.strides)[...] = True
    assert (buf[~inside] == 255).all() and buf.size >= case.offset + case.batch * case.batch_stride


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_row_takes_its_path_and_keeps_the_oracle_keys(name):
    """row_path against the label (named_path, the paths by their conditions) on image 0, and against O.kstrongest's kept
    keys on every row of every image; the first row keeps bins within 3 bins of both row ends (the peak scores use the halo)."""
    case = K.CASES[name]
    img = _images(name)
    for b in range(case.batch):
        want = _oracle_keys(img[b], case.k, case.z_min)
        for r in range(case.rows):
            path, keys, _ = K.row_path(img[b, r], case.k, case.z_min)
            if b == 0:
                assert path == case.recipes[r].path, (name, r, case.recipes[r], path)
            assert path == K.named_path(img[b, r], case.k, case.z_min), (name, b, r)
            np.testing.assert_array_equal(keys, want[r], err_msg="%s image %d row %d (%s)" % (name, b, r, path))
        if case.recipes[0].kind == "random" and case.k >= 5 and case.cols >= 16:
            # (with uchar(z_min) = 255 every candidate is 255 and ties go to the larger range: only the far end is kept)
            bins = [int(x) & 0xFFFFFF for x in want[0]]
            assert (min(bins) <= 3 or K.u_zmin(case.z_min) == 255) and max(bins) >= case.cols - 4, (name, b, min(bins), max(bins))


def test_every_instantiation_and_every_path_has_a_case(capsys):
    reached, per_chunk, cuts = {}, {}, set()
    mask_ragged, bytes_paths = set(), set()
    for case in K.CASES.values():
        reached.setdefault(K.table_index(*case.inst), []).append(case.name)
        img = _images(case.name)
        for r, row in enumerate(case.recipes):
            per_chunk.setdefault((case.inst[0], row.path), []).append((case.name, r))
            if case.inst[2] and case.cols % 16:
                mask_ragged.add(row.path)
            if not case.inst[1]:
                bytes_paths.add(row.path)
            T = K.row_path(img[0, r], case.k, case.z_min)[2]
            if T is not None:
                cuts.add(T >= 128)
    with capsys.disabled():
        print()
        for i in range(16):
            print("  table %2d %-20s %2d cases, e.g. %s" % (i, K.entry_name(i), len(reached.get(i, [])), ", ".join(reached.get(i, [])[:2])))
        for n in K.NCHUNKS:
            for path in K.PATHS:
                rows = per_chunk.get((n, path), [])
                print("  NCHUNK %d %-22s %3d rows, e.g. %s row %d" % ((n, path, len(rows)) + (rows[0] if rows else ("-", -1))))
    assert sorted(reached) == list(range(16))
    for n in K.NCHUNKS:
        assert {p for (c, p) in per_chunk if c == n} == set(K.PATHS), n
    assert mask_ragged >= set(K.DENSE_PATHS), set(K.DENSE_PATHS) - mask_ragged
    assert bytes_paths >= set(K.DENSE_PATHS), set(K.DENSE_PATHS) - bytes_paths
    assert cuts == {False, True}                            # cut intensities on both sides of 128: both forms of the byte compare
    # every instantiation at k = 12, 65 and 300; the whole k list on an NCHUNK 1 and an NCHUNK 4 layout; the threshold lists
    by_inst = {}
    for case in K.CASES.values():
        by_inst.setdefault(case.inst, set()).add(case.k)
    assert all(ks >= set(K.K_FEW) for ks in by_inst.values()) and len(by_inst) == 16
    for prefix in ("klist-n1-", "klist-n4-"):
        assert {c.k for c in K.CASES.values() if c.name.startswith(prefix)} == set(K.K_ALL)
    assert {c.z_min for c in K.CASES.values() if c.inst[2]} == set(K.Z_MASK)
    assert {c.z_min for c in K.CASES.values() if not c.inst[2]} >= set(K.Z_PLAIN)
    widths = {c.cols for c in K.CASES.values()}
    assert widths >= {300, 1024, 1025, 2048, 2049, 3768, 4096, 4097, 8191, 8192} | set(K.NARROW)
    layouts = {(c.offset % 4, c.stride % 4 == 0, c.batch, c.batch_stride % 4 == 0, c.stride > c.cols) for c in K.CASES.values()}
    assert {o for o, *_ in layouts} == {0, 1, 2, 3} and any(c.stride % 2 for c in K.CASES.values())
    assert any(c.batch == 2 and c.batch_stride % 4 for c in K.CASES.values())
    assert any(c.batch == 3 and c.batch_stride == c.rows * c.stride + 16 and c.inst[1] for c in K.CASES.values())
    assert any(c.stride == (c.cols + 15) // 16 * 16 + 16 for c in K.CASES.values())
    for cols in K.NARROW[:-1]:
        assert {c.stride for c in K.CASES.values() if c.cols == cols} == {cols, 16}
    assert any(c.cols % 16 == 8 and c.stride == c.cols and c.inst[1] for c in K.CASES.values())    # a byte-gathered last piece on the vector path


def test_witness_of_the_bracketing_order():
    """row = arange(1024) % 256, z_min = 0, k = 300: the first trial passes 284 bins (256 < 284 < k).  Tested for "> 256" first,
    as the kernel did, the loop raises lo past the cut and ends at T = 191 with 260 keys; tested for "< k" first it ends
    exactly, c_lo >= k > c_hi, on the oracle's cut intensity 181.  k = 257 on the same row comes out right either way."""
    case = K.CASES[K.WITNESS]
    row = _images(K.WITNESS)[0, 0]
    np.testing.assert_array_equal(row, np.arange(1024) % 256)
    want = _oracle_keys(row[None], case.k, case.z_min)[0]
    assert want.size == 300 and int(want[0] >> 24) == 181
    path, keys, T = K.row_path(row, case.k, case.z_min)
    assert (path, T) == ("bracket+tiescan_exact", 181)
    np.testing.assert_array_equal(keys, want)
    path, keys, T = K.row_path(row, case.k, case.z_min, parent_order=True)
    assert (path, T, keys.size) == ("bracket+tiescan_exact", 191, 260)
    for order in (False, True):
        np.testing.assert_array_equal(K.row_path(row, 257, 0, parent_order=order)[1], _oracle_keys(row[None], 257, 0)[0])


def test_model_equals_the_oracle_on_a_random_sweep():
    """1600 seeded rows over widths, k up to 1024 and the threshold lists, of four kinds (uniform noise, exponential clutter
    with returns, few levels -- wide plateaux --, a ramp): the kept keys are the oracle's, the path is the named one, and for
    k <= 256 the comparison order of the bracketing loop makes no difference (the fix changes no such row)."""
    rng = np.random.default_rng(20260)
    widths = (17, 64, 65, 200, 256, 257, 300, 1000, 1024, 1025, 2049, 3768, 4100, 8192)
    ks = (1, 3, 12, 40, 64, 65, 100, 255, 256, 257, 300, 511, 1024)
    paths, differs = collections.Counter(), 0
    for i in range(1600):
        cols, k, z = int(rng.choice(widths)), int(rng.choice(ks)), float(rng.choice(K.Z_MASK + K.Z_PLAIN))
        kind = i % 4
        if kind == 0:
            row = rng.integers(0, 256, cols)
        elif kind == 1:
            row = (6 + rng.exponential(float(rng.choice([12.0, 40.0, 90.0])), cols)).clip(0, 255)
        elif kind == 2:
            row = rng.choice(rng.integers(0, 256, int(rng.integers(1, 6))), cols)
        else:
            row = (np.arange(cols) * int(rng.integers(1, 5)) + int(rng.integers(0, 256))) % 256
        row = row.astype(np.uint8)
        path, keys, _ = K.row_path(row, k, z)
        want = _oracle_keys(row[None], k, z)[0]
        np.testing.assert_array_equal(keys, want, err_msg="row %d: cols %d k %d z_min %g (%s)" % (i, cols, k, z, path))
        assert path == K.named_path(row, k, z), (i, cols, k, z)
        paths[path] += 1
        old = K.row_path(row, k, z, parent_order=True)[1]
        if k <= 256:
            np.testing.assert_array_equal(old, keys)
        elif old.size != keys.size or (old != keys).any():
            differs += 1
    assert set(paths) == set(K.PATHS) and differs > 0, (paths, differs)


def test_plan_invariants_over_a_sweep():
    """cols 1..8192 x base mod 4 x stride mod 4 x batch stride mod 4 x z_min: nchunk covers cols with the smallest chunk count,
    vec holds iff base, stride and batch stride are multiples of 4, mask iff uchar((int)z_min) == 0, the index is the
    header's formula, and the LDS stays inside the 64 KiB a launch gets without asking (so inside the CU's 160 KiB)."""
    import ctypes as C
    from tbv_slam_public_amd import _lib as L
    lib = L.lib()
    d, out = L.PolarDesc(), L.KStrongPlan()
    zs = K.Z_MASK + K.Z_PLAIN
    seen = set()
    for cols in range(1, 8193):
        for base in range(4):
            smod, bmod = (cols + base) % 4, (cols // 4 + base) % 4       # all 16 (stride, batch stride) residues come by over the widths
            z = zs[(cols + base) % len(zs)]
            k = (1, 12, 64, 65, 300, 1024)[(cols // 3 + base) % 6]
            stride = cols + (smod - cols) % 4
            d.rows, d.cols, d.stride, d.batch = 7, cols, stride, 2
            d.batch_stride = 7 * stride + (bmod - 7 * stride) % 4
            par = L.KStrongParams(k, float(z), K.RANGE_RES, 2.5, 1)
            assert lib.cfear_kstrong_plan(C.byref(d), C.byref(par), 0x7f0000001000 + base, C.byref(out)) == 0 and out.refused == 0
            assert out.nchunk in K.NCHUNKS and out.nchunk * 1024 >= cols and (out.nchunk == 1 or out.nchunk * 512 < cols)
            assert out.vec == int(base == 0 and smod == 0 and bmod == 0), (cols, base, smod, bmod)
            assert out.mask == int(K.u_zmin(z) == 0) and out.u_zmin == K.u_zmin(z) and out.thi == int(out.u_zmin >= 128)
            assert out.table_index == K.table_index(out.nchunk, out.vec, out.mask)
            kpad = max((k + 3) // 4 * 4, 64)
            scratch = max(1024, ((out.nchunk + 1) // 2 + 2) * 256)
            assert out.kpad == kpad and out.lds_bytes == 4 * (out.nchunk * 1024 + 32 + scratch + 4 * kpad) <= 64 * 1024
            seen.add((out.table_index, smod, bmod, base))
    assert {i for i, *_ in seen} == set(range(16)) and len({s[1:] for s in seen}) == 64
    assert K.u_zmin(256) == 0 and K.u_zmin(0.9) == 0 and K.u_zmin(300) == 44 and K.u_zmin(-1) == 255
    # a single image's batch stride does not count
    from tbv_slam_public_amd import api
    assert api.kstrong_plan(7, 1024, 12, 60, batch=1, batch_stride=7 * 1024 + 1)["vec"] == 1
    assert api.kstrong_plan(7, 1024, 12, 60, batch=2, batch_stride=7 * 1024 + 1)["vec"] == 0


def test_plan_reports_what_the_filter_refuses():
    from tbv_slam_public_amd import api, _lib as L
    ok = dict(rows=7, cols=300, k=12, z_min=60)
    assert api.kstrong_plan(**ok)["refused"] is None
    assert api.kstrong_plan(**{**ok, "k": 1024})["refused"] is None and api.kstrong_plan(**{**ok, "cols": 8192})["refused"] is None
    for bad, why in ((dict(k=0), "k_strongest"), (dict(k=1025), "k_strongest"), (dict(cols=8193), "cols"), (dict(rows=0), "descriptor"),
                     (dict(cols=0), "descriptor"), (dict(stride=299), "descriptor"), (dict(batch=0), "descriptor"),
                     (dict(batch=2, batch_stride=7 * 300 - 1), "descriptor"), (dict(range_res=0.0), "range_res")):
        p = api.kstrong_plan(**{**ok, **bad})
        assert p["refused"] and why in p["refused"], (bad, p)
        assert all(v == 0 for name, v in p.items() if name != "refused"), p
    assert L.lib().cfear_kstrong_plan(None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    import ctypes as C
    assert C.sizeof(L.KStrongPlan) == 48                    # struct cfear_kstrong_plan: ten int32 and one int64
