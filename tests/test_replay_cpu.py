"""CPU: tests/replay_cpu.py -- the replay's state rules restated from the oracle's primitives -- pinned against the oracle's
own fuser: replaying the trace O.Fuser produced on a fuser drive reproduces that fuser frame by frame.  The restatement
feeds the same functions the same inputs, so the counts are equal and the deviation from the trace is exactly zero."""
import numpy as np

from tests import fuser_cases as FC
from tests import replay_cpu as RC
from tests.test_fuser_cases_cpu import make_oracle

OVERRIDES = dict(min_keyframe_dist=1.0)          # a keyframe every second frame of STRAIGHT (0.6 m per frame)


def _fuser_run(poses, overrides):
    fz = make_oracle(overrides)
    clouds = [FC.cloud(FC.WORLDS["unit"], pose, f) for f, pose in enumerate(poses)]
    out = []
    for c in clouds:
        pose, info = fz.process(c)
        out.append(dict(pose=pose.copy(), n_cells=int(info[0]), keyframe=int(info[1]), ok=int(info[2]), iters=int(info[3]),
                        replaced=fz.last_decision()["replaced"]))
    return clouds, out


def test_replay_of_the_fusers_own_trace_reproduces_the_fuser():
    clouds, live = _fuser_run(FC.STRAIGHT, OVERRIDES)
    trace = np.array([r["pose"] for r in live])
    rec = RC.replay(clouds, trace, OVERRIDES)
    flags = [r["is_keyframe"] for r in rec]
    assert flags == [r["keyframe"] for r in live]
    assert 0 in flags[1:] and 1 in flags[1:]                                 # a frame that is a keyframe and one that is not
    assert sum(flags) > RC.params(OVERRIDES)["submap_scan_size"]             # ... and more keyframes than the window holds:
    assert rec[-1]["window"][0] > 0 and len(rec[-1]["window"]) == 4          # the window has started to slide
    assert np.array_equal(RC.keyframe_flags(trace, RC.params(OVERRIDES)), flags)
    for t, (r, want) in enumerate(zip(rec, live)):
        assert r["n_cells"] == want["n_cells"], t
        if t == 0:
            assert r["first"] and r["n_targets"] == 0
            continue
        assert (r["ok"], r["outer_iters"]) == (want["ok"], want["iters"]), t
        assert r["sanity_ok"] == int(not want["replaced"]), t
        assert r["n_targets"] == min(4, sum(flags[:t])), t
        print(t, "dev", r["dev"], "pose - trace", r["pose"] - trace[t])
        assert not r["dev"].any(), (t, r["dev"])                             # exactly zero


def test_a_perturbed_trace_changes_only_the_frames_that_read_it():
    """Locality on the CPU: a perturbed non-keyframe pose P_j changes frames j (its dev), j + 1 and j + 2 (their motion: the
    compensation and the guess) only -- where neither of the two is a keyframe, whose compensated scan later windows would
    hold.  A keyframe every fourth frame (2 m at 0.6 m per frame), j = 5."""
    over = dict(min_keyframe_dist=2.0)
    clouds, live = _fuser_run(FC.straight(12, 0.6), over)
    trace = np.array([r["pose"] for r in live])
    base = RC.replay(clouds, trace, over)
    flags = [r["is_keyframe"] for r in base]
    j = 5
    assert sum(flags) >= 3 and not flags[j] and not flags[j + 1] and not flags[j + 2]
    bent = trace.copy()
    bent[j] += (0.05, 0.0, 0.002)
    assert np.array_equal(RC.keyframe_flags(bent, RC.params(over)), flags)
    got = RC.replay(clouds, bent, over)
    for t in range(len(trace)):
        same = np.array_equal(got[t]["pose"], base[t]["pose"]) and np.array_equal(got[t]["dev"], base[t]["dev"])
        if t == j:
            assert np.array_equal(got[t]["pose"], base[t]["pose"]) and not np.array_equal(got[t]["dev"], base[t]["dev"])
        elif t in (j + 1, j + 2):
            assert not same, t
        else:
            assert same, t
