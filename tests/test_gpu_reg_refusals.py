"""GPU: what the registration family's entry points answer to a malformed job, scan handle or candidate -- status, the
whole cfear_last_error text, and outputs left alone.  Every case is refused on the host before anything is launched.

The entry points share one scan check and one job check (cfear_reg_check_scan / cfear_reg_check_job, csrc/register.hip); the
tie audit words its refusals "job <j>: ..." and also wants finite poses, the matcher's entry points do neither, and when a
job has two faults the first one in scan order is named.  The literals in EXPECTED were recorded from the library as it was
before the checks were folded into those two functions, and pin that.

Two 3-scan jobs and a 2-scan job over constructed scans of a few dozen cells (tests/tieaudit_cpu.py::_job); the fault always
sits in the middle job.  A fault is left out for an entry point that does not look for it (a job's null `scans` or
`poses_xyt` is the caller's to avoid in the matcher's batch entry points; only the audit checks them)."""
import ctypes as C

import numpy as np
import pytest

from tests import tieaudit_cpu as R

pytestmark = pytest.mark.gpu

FILL = 0x5A
NAN = float("nan")

# fault -> what it does to the middle job: (n_scans or None, {scan: handle}, {(scan, k): pose value}, null scans, null poses)
# handle: None = a null handle, "foreign" = a scan of a second context
FAULTS = {
    "n_scans 1": (1, {}, {}, False, False),
    "n_scans 17": (17, {}, {}, False, False),
    "null first handle": (None, {0: None}, {}, False, False),
    "null last handle": (None, {2: None}, {}, False, False),
    "scan of another context": (None, {1: "foreign"}, {}, False, False),
    "null scans": (None, {}, {}, True, False),
    "null poses": (None, {}, {}, False, True),
    "nan pose 0, null handle 1": (None, {1: None}, {(0, 2): NAN}, False, False),
    "null handle 0, nan pose 1": (None, {0: None}, {(1, 0): NAN}, False, False),
}
JOB_FAULTS = ["n_scans 1", "n_scans 17", "null first handle", "null last handle", "scan of another context"]
ARGUMENT_FAULTS = ["null scans", "null poses"]
AUDIT_ONLY = ["nan pose 0, null handle 1", "null handle 0, nan pose 1"]
CASES = {
    "cfear_register_batch": JOB_FAULTS,
    "cfear_get_cost_batch": JOB_FAULTS,
    "cfear_covariance_by_sampling_batch": JOB_FAULTS,
    "cfear_association_ties_batch": JOB_FAULTS + ARGUMENT_FAULTS + AUDIT_ONLY,
    "cfear_register": JOB_FAULTS + ARGUMENT_FAULTS,
    "cfear_cost_prepare": JOB_FAULTS + ARGUMENT_FAULTS,
    "cfear_scan_table_create": ["null first handle", "null last handle", "scan of another context", "null scans"],
    "cfear_register_candidates": ["source index = table size"],
}

INV = -1                                        # CFEAR_ERR_INVALID_ARGUMENT (asserted below)
N_SCANS = "n_scans must be in [2,16]"
HANDLE, CONTEXT = "null scan handle", "scan belongs to another context"
_MATCHER = {"n_scans 1": (INV, N_SCANS, "untouched"), "n_scans 17": (INV, N_SCANS, "untouched"),
            "null first handle": (INV, HANDLE, "untouched"), "null last handle": (INV, HANDLE, "untouched"),
            "scan of another context": (INV, CONTEXT, "untouched")}
EXPECTED = {
    "cfear_register_batch": _MATCHER,
    "cfear_get_cost_batch": _MATCHER,
    "cfear_covariance_by_sampling_batch": _MATCHER,
    "cfear_association_ties_batch": {
        "n_scans 1": (INV, "job 1: " + N_SCANS, "untouched"), "n_scans 17": (INV, "job 1: " + N_SCANS, "untouched"),
        "null first handle": (INV, "job 1: " + HANDLE, "untouched"), "null last handle": (INV, "job 1: " + HANDLE, "untouched"),
        "scan of another context": (INV, "job 1: " + CONTEXT, "untouched"),
        "null scans": (INV, "job 1: null scans or poses", "untouched"), "null poses": (INV, "job 1: null scans or poses", "untouched"),
        "nan pose 0, null handle 1": (INV, "job 1: pose 0 is not finite", "untouched"),
        "null handle 0, nan pose 1": (INV, "job 1: " + HANDLE, "untouched"),
    },
    "cfear_register": dict(_MATCHER, **{"null scans": (INV, "null argument", "untouched"), "null poses": (INV, "null argument", "untouched")}),
    # the handle is cleared once the arguments are there, before the job is looked at
    "cfear_cost_prepare": dict({k: v[:2] + ("handle cleared",) for k, v in _MATCHER.items()},
                               **{"null scans": (INV, "null argument", "untouched"), "null poses": (INV, "null argument", "untouched")}),
    "cfear_scan_table_create": {
        "null first handle": (INV, HANDLE, "handle cleared"), "null last handle": (INV, HANDLE, "handle cleared"),
        "scan of another context": (INV, CONTEXT, "handle cleared"), "null scans": (INV, "null argument / empty table", "untouched"),
    },
    "cfear_register_candidates": {"source index = table size": (INV, "candidate 1 refers to scan 0 / 3 of a table of 3", "untouched")},
}


class Scene:
    """The three jobs on the device, a scan of a second context, and the middle job with a fault built in."""

    def __init__(self):
        from tbv_slam_public_amd import api, _lib as L
        self.api, self.L = api, L
        self.ctx = api.default_context()
        self.other = api.Context()
        rng = np.random.default_rng(20261021)
        host = [R._job(rng, 3, 40), R._job(rng, 3, 33), R._job(rng, 2, 24)]
        self.jobs = [([api.MapPointNormal(cells=c) for c in scans], np.ascontiguousarray(poses, np.float64)) for scans, poses in host]
        self.foreign = api.MapPointNormal(cells=host[1][0][1], ctx=self.other)
        self.reg = api.n_scan_normal_reg()
        self.total = sum(len(c[-1]) * (len(c) - 1) for c, _ in host)

    def middle(self, fault):
        """(handles, n_scans, poses, null scans, null poses) of the middle job with the fault"""
        n_scans, handles, poses, null_scans, null_poses = FAULTS[fault]
        scans, T = self.jobs[1]
        hs = (C.c_void_p * len(scans))(*[s._h for s in scans])
        for i, h in handles.items():
            hs[i] = self.foreign._h if h == "foreign" else None
        T = T.copy()
        for (i, k), v in poses.items():
            T[i, k] = v
        return hs, (n_scans or len(scans)), T, null_scans, null_poses

    def batch(self, fault):
        arr, n, keep = self.reg.PrepareBatch(self.jobs)
        hs, n_scans, T, null_scans, null_poses = self.middle(fault)
        arr[1].scans = None if null_scans else C.cast(hs, C.POINTER(C.c_void_p))
        arr[1].n_scans = n_scans
        arr[1].poses_xyt = None if null_poses else T.ctypes.data_as(C.POINTER(C.c_double))
        return arr, n, (keep, hs, T)


def _filled(nbytes):
    return np.full(nbytes, FILL, np.uint8)


def _state(*buffers):
    return "untouched" if all((b == FILL).all() for b in buffers) else "written"


def _handle_state(h):
    return "untouched" if h.value == int.from_bytes(bytes([FILL]) * 8, "little") else ("handle cleared" if not h.value else "handle set")


def collect():
    """{entry point: {fault: (status, cfear_last_error, what became of the outputs)}}"""
    s = Scene()
    L, lib, ctx = s.L, s.ctx._lib, s.ctx
    par = C.byref(s.reg.par)
    dp = C.POINTER(C.c_double)
    got = {name: {} for name in CASES}

    def note(name, fault, rc, state):
        got[name][fault] = (int(rc), lib.cfear_last_error(ctx.h).decode(), state)

    for fault in JOB_FAULTS + ARGUMENT_FAULTS + AUDIT_ONLY:
        arr, n, keep = s.batch(fault)
        if fault in CASES["cfear_register_batch"]:
            res = _filled(n * 72)
            note("cfear_register_batch", fault, lib.cfear_register_batch(ctx.h, arr, n, par, res.ctypes.data), _state(res))
            res = _filled(n * 72)
            note("cfear_get_cost_batch", fault, lib.cfear_get_cost_batch(ctx.h, arr, n, par, res.ctypes.data), _state(res))
            regs = np.zeros(n, L.RESULT_DTYPE)
            sp = s.reg.sampling_params()
            cov, smp, ok = _filled(n * 36 * 8), _filled(n * 27 * 4 * 8), _filled(n * 4)
            rc = lib.cfear_covariance_by_sampling_batch(ctx.h, arr, n, par, regs.ctypes.data, C.byref(sp), cov.ctypes.data, smp.ctypes.data,
                                                        ok.ctypes.data)
            note("cfear_covariance_by_sampling_batch", fault, rc, _state(cov, smp, ok))
        rec, pq = _filled(n * 32), _filled(s.total * 12)
        rc = lib.cfear_association_ties_batch(ctx.h, arr, n, par, 1, rec.ctypes.data, pq.ctypes.data, s.total)
        note("cfear_association_ties_batch", fault, rc, _state(rec, pq))
        if fault in CASES["cfear_register"]:
            hs, n_scans, T, null_scans, null_poses = s.middle(fault)
            before = T.copy()
            res = _filled(72)
            rc = lib.cfear_register(ctx.h, None if null_scans else hs, n_scans, None if null_poses else T.ctypes.data_as(dp), par,
                                    C.cast(res.ctypes.data, C.POINTER(L.RegResult)))
            note("cfear_register", fault, rc, _state(res) if np.array_equal(T, before, equal_nan=True) else "poses written")
            out = C.c_void_p(int.from_bytes(bytes([FILL]) * 8, "little"))
            rc = lib.cfear_cost_prepare(ctx.h, None if null_scans else hs, n_scans, None if null_poses else T.ctypes.data_as(dp), par, 0,
                                        C.byref(out))
            note("cfear_cost_prepare", fault, rc, _handle_state(out))
        if fault in CASES["cfear_scan_table_create"]:
            hs, n_scans, T, null_scans, null_poses = s.middle(fault)
            out = C.c_void_p(int.from_bytes(bytes([FILL]) * 8, "little"))
            note("cfear_scan_table_create", fault, lib.cfear_scan_table_create(ctx.h, None if null_scans else hs, n_scans, C.byref(out)),
                 _handle_state(out))

    table = s.api.ScanTable(s.jobs[1][0])
    cands = s.api.ScanTable.candidates([0, 0], [1, len(table)], np.zeros((2, 3)))
    res = _filled(2 * 72)
    rc = lib.cfear_register_candidates(ctx.h, table._h, C.c_void_p(cands.ctypes.data), 2, par, res.ctypes.data)
    note("cfear_register_candidates", "source index = table size", rc, _state(res))
    # the scene is sound: the same calls without a fault go through
    arr, n, keep = s.reg.PrepareBatch(s.jobs)
    res = _filled(n * 72)
    assert lib.cfear_register_batch(ctx.h, arr, n, par, res.ctypes.data) == L.OK and _state(res) == "written"
    rec, pq = _filled(n * 32), _filled(s.total * 12)
    assert lib.cfear_association_ties_batch(ctx.h, arr, n, par, 1, rec.ctypes.data, pq.ctypes.data, s.total) == L.OK
    cands["source"][1] = 2
    assert lib.cfear_register_candidates(ctx.h, table._h, C.c_void_p(cands.ctypes.data), 2, par, res.ctypes.data) == L.OK
    table.close()
    del s.foreign
    s.other.close()
    return got


def test_malformed_jobs_scans_and_candidates_are_refused_as_before():
    from tbv_slam_public_amd import _lib as L
    assert L.ERR_INVALID_ARGUMENT == INV
    got = collect()
    assert {k: sorted(v) for k, v in got.items()} == {k: sorted(v) for k, v in CASES.items()}
    for name in CASES:
        for fault in CASES[name]:
            print(name, "|", fault, "|", got[name][fault])
            assert got[name][fault] == EXPECTED[name][fault], (name, fault, got[name][fault], EXPECTED[name][fault])
