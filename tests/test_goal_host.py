"""CPU: the host side of the torque-aware goal search -- the restatement in tests/goal_ref.py
(whose cases() asserts the margins and the coverage of the shared case set), ik.free_grid, the
Problem switch and the GoalStats mirror.  No compute call of libtcmp.so is made here."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import oracle as O  # noqa: E402  (test infrastructure)
import goal_ref as G


@pytest.fixture(scope="module")
def shared():
    return G.cases()


def test_case_set_margins_and_coverage(shared):
    """cases() asserted them; the set is the issue's: seven cases over five poses."""
    out, free, ref, obs = shared
    assert [name for name, _, _, _ in out] == ["p22_dyn", "p25_dyn", "p17_dyn", "p17_rne",
                                               "p4_dyn", "p2_dyn", "far_dyn"]
    assert len(free) == 32 and obs.shape == (16, 15)
    by = {name: G.counts(r) for name, _, _, r in out}
    # the issue's probe figures for the poses it names
    assert by["p22_dyn"][1:] == (12, 10, 4)
    assert by["p17_dyn"][1:] == (18, 0, 0) and by["p17_rne"][1:] == (18, 0, 0)
    assert by["p4_dyn"][3] == 0 < by["p4_dyn"][2]


def test_counts_monotone_and_rows(shared):
    out, free, ref, obs = shared
    for name, T, mode, r in out:
        c = G.counts(r)
        assert c[0] >= c[1] >= c[2] >= c[3] >= 0, name
        assert r["n_out"] == min(c[3], 8) == len(r["rows"])
        assert r["base_collides"] == 0
        for i, q, d, h in r["feasible"]:
            assert q[6] == free[i // 8], (name, i)         # joint 7 is the free value, bitwise
            assert np.abs(O.fk8(q) - T).max() < 1e-9, (name, i)
            assert d == G.distance(ref, q, np.full(7, 10.0))
            assert 0.0 < h <= 1.0
        keys = [(d, i) for i, _, d, _ in r["feasible"]]
        assert keys == sorted(keys), name
        assert len({i for _, i in keys}) == len(keys)


def test_max_out_one_is_the_argmin(shared):
    out, free, ref, obs = shared
    for name, T, mode, r in out:
        one = G.search(T, free, ref, obs, mode, G.MASS, None, 1)
        assert G.counts(one) == G.counts(r)
        if not r["n_feasible"]:
            assert one["rows"] == [] and one["n_out"] == 0
            continue
        best = min(r["feasible"], key=lambda row: (row[2], row[0]))
        assert one["n_out"] == 1 and one["rows"][0][0] == best[0]
        assert (one["rows"][0][1] == best[1]).all()


def test_headroom_is_not_an_order(shared):
    """Base mode: every in-limit candidate passes with headroom 1.0."""
    out, free, ref, obs = shared
    _, T, _, r = out[0]
    b = G.search(T, free, ref, obs, G.BASE, G.MASS)
    assert b["n_torque_ok"] == b["n_in_limits"] == r["n_in_limits"]
    assert all(h == 1.0 for _, _, _, h in b["feasible"])


def test_weights_change_the_order(shared):
    out, free, ref, obs = shared
    _, T, mode, r = out[1]
    w = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 400.0])
    v = G.search(T, free, ref, obs, mode, G.MASS, w, 64)
    assert sorted(i for i, _, _, _ in v["feasible"]) == sorted(i for i, _, _, _ in r["feasible"])
    for i, q, d, _ in v["feasible"]:
        assert d == G.distance(ref, q, w)


def test_joint6_image_rule():
    """Only q6 below the lower limit whose +2 pi image is at most the upper one moves."""
    q = np.array([0.1, 0.2, 0.3, -1.0, 0.4, 0.0, 0.5])
    for q6, want in ((-2.6, -2.6 + 2 * np.pi), (-np.pi + 1e-9, np.pi + 1e-9),
                     (3.7525 - 2 * np.pi - 1e-12, 3.7525 - 2 * np.pi - 1e-12 + 2 * np.pi),
                     (-2.5, -2.5), (-0.0175, -0.0175), (-0.02, -0.02), (1.0, 1.0), (3.0, 3.0)):
        q[5] = q6
        got = G.joint6_image(q)
        assert got[5] == want and (got[[0, 1, 2, 3, 4, 6]] == q[[0, 1, 2, 3, 4, 6]]).all()
        assert q[5] == q6                                   # the input is left alone
    assert -2.5 + 2 * np.pi > G.HI[5]                       # the image is unique


def test_wide_joint6_goals_are_found():
    """The generating q (q6 above pi) is a feasible row of every case: wide_cases() asserts it.
    Without the image rule the limit filter drops it: tcmp_ik reports it at q6 - 2 pi."""
    qs, poses, out = G.wide_cases()
    assert [(s, m) for s, _, m, _ in out] == [("empty", G.BASE), ("empty", G.RNE),
                                              ("box16", G.BASE), ("box16", G.RNE)]
    for q, T in zip(qs, poses):
        sols, _ = O.ik8(T, q[6])
        k = int(np.argmin(np.abs((sols - q + np.pi) % (2 * np.pi) - np.pi).max(axis=1)))
        assert abs(sols[k, 5] - (q[5] - 2 * np.pi)) < 1e-8 and sols[k, 5] < G.LO[5]
    for sname, obs, mode, rs in out:
        for q, r in zip(qs, rs):
            c = G.counts(r)
            assert c[0] >= c[1] >= c[2] >= c[3] > 0, (sname, mode)
            assert any(row[1][5] > np.pi for row in r["feasible"])
            for i, cq, d, h in r["feasible"]:
                assert (G.LO <= cq).all() and (cq <= G.HI).all()


def test_ik_candidates_keeps_the_reported_angle():
    """The difference, on purpose: the drop-in path ik.ik_candidates replays the reference, which
    filters on the angle as reported ((-pi, pi]) and so loses the goals joint 6's image holds;
    the goal search alone takes the image."""
    from torque_constrained_motion_planning_amd import ik as IK
    from test_ik_host import OracleEngine
    qs, poses, out = G.wide_cases()
    rs = out[0][3]                                           # empty scene, base mode
    lost = 0
    for q, T, r in zip(qs, poses, rs):
        np.random.seed(1)
        flat = IK.ik_candidates(OracleEngine(), T @ IK.EE_TO_TOOL, q, max_attempts=1,
                                shuffle=lambda c: None)
        assert all(c[5] <= np.pi for c in flat)
        assert not any(np.abs(c - q).max() <= 1e-8 for c in flat)
        wide = [row for row in r["feasible"] if row[0] < 8 and row[1][5] > np.pi]
        assert wide                                          # free value 0 = q7: the search has them
        lost += len(wide)
    assert lost >= len(qs)


def test_free_grid():
    from torque_constrained_motion_planning_amd import ik as IK
    from torque_constrained_motion_planning_amd.scene import JOINT_LOWER, JOINT_UPPER
    lo7, hi7 = float(JOINT_LOWER[6]), float(JOINT_UPPER[6])
    for cur, n in ((0.25, 1), (-1.5, 2), (np.pi / 4, 32), (0.0, 257)):
        g = IK.free_grid(cur, n)
        assert g.dtype == np.float64 and g.shape == (n,)
        assert g[0] == cur
        for i in range(n - 1):
            assert g[1 + i] == lo7 + (i + 0.5) / (n - 1) * (hi7 - lo7)
        assert ((g[1:] > lo7) & (g[1:] < hi7)).all()
        assert (np.diff(g[1:]) > 0).all()
    with pytest.raises(ValueError):
        IK.free_grid(0.0, 0)


def test_problem_switch_defaults_off():
    from torque_constrained_motion_planning_amd.utils import Problem
    p = Problem(None, [], None, 5.0, 1.0)
    assert p.goal_search is False
    assert Problem(None, [], None, 5.0, 1.0, goal_search=32).goal_search == 32
    kind = inspect.signature(Problem.__init__).parameters["goal_search"].kind
    assert kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(TypeError):
        Problem(None, [], None, 5.0, 1.0, "arne", False, False, True)


def test_goal_search_for_pose_signature():
    from torque_constrained_motion_planning_amd import ik as IK
    sig = inspect.signature(IK.goal_search_for_pose)
    assert list(sig.parameters) == ["problem", "start_conf", "pose", "torque_test", "n_free",
                                    "engine"]
    assert sig.parameters["n_free"].default == 256


def test_goal_stats_layout(tmp_path):
    """ctypes.sizeof(GoalStats) is the C size, and the fields sit where the header puts them."""
    from torque_constrained_motion_planning_amd import _lib
    src = tmp_path / "goal_sizes.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "tcmp.h"
int main(void) { printf("%zu %zu %zu %zu\n", sizeof(tcmp_goal_stats), offsetof(tcmp_goal_stats, n_feasible), offsetof(tcmp_goal_stats, n_out), offsetof(tcmp_goal_stats, base_collides)); return 0; }
''')
    exe = str(tmp_path / "goal_sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    size, o_feas, o_out, o_base = map(int, subprocess.check_output([exe]).split())
    S = _lib.GoalStats
    assert size == ctypes.sizeof(S) == 40
    assert (o_feas, o_out, o_base) == (S.n_feasible.offset, S.n_out.offset, S.base_collides.offset)
    assert "tcmp_goal_search" in _lib.EXPORTS
