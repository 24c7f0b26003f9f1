"""GPU half of the boundary tests of the triangulation, Sim3 and pose ports: every boundary problem of
tests/geometry_boundary_worlds.py through the device call (orbv_triangulate_pairs, orbm_sim3_ransac, orbm_pose_optimize), every
record, mask word and flag byte for byte against the library's host routine in device order.  The worlds are built on the CPU and
checked there (tests/test_geometry_boundary_worlds.py); a mismatch is reported by the groups and sides of the cases that differ."""
import numpy as np
import pytest

import geometry_boundary_worlds as gb
import pose_worlds as pw
import sim3_worlds as sw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


@pytest.fixture(scope="module")
def search():
    import multi_orb_slam_amd as m
    S = m.BowSearch()
    yield S
    S.close()


def test_the_worlds_meet_their_conditions():
    print(gb.check_conditions()[0])


# ---- triangulation -----------------------------------------------------------------------------------------------------------------------
def kinds_of_differences(got, want, groups, sides):
    """The groups (with sides) of the pairs whose records differ."""
    bad = [p for p in range(len(want)) if got[p].tobytes() != want[p].tobytes()]
    return sorted({"%s[%s]" % (groups[p], sides[p]) for p in bad})


def test_triangulation_boundaries(search):
    differing = []
    for (name, w, groups, sides), host in zip(gb.tri_worlds(), gb.tri_host()):
        got = w.device(search)
        assert len(got) == len(host)
        differing += ["%s: %s" % (name, k) for k in kinds_of_differences(got, host, groups, sides)]
    assert not differing, differing


def test_triangulation_boundaries_at_every_batch_position(search):
    """Every world once per group of it, with members of that group at positions 0, 63 and 64 of the launch (a world of fewer than
    66 pairs repeated to that length: the side worlds' single pairs stand on every lane of the first wave and on the first of the
    second)."""
    worlds, host = gb.tri_worlds(), gb.tri_host()
    orders = gb.batch_orders()
    assert {g for _, g, _ in orders} == {g for _, _, groups, _ in worlds for g in groups}
    differing = []
    for wi, g, order in orders:
        _, w, groups, sides = worlds[wi]
        got = w.device(search, w.pairs[order])
        assert len(got) == len(order) > 65
        diff = kinds_of_differences(got, host[wi][order], [groups[k] for k in order], [sides[k] for k in order])
        differing += ["%s in the order for %s" % (d, g) for d in diff]
    assert not differing, differing


# ---- Sim3 --------------------------------------------------------------------------------------------------------------------------------
def sim3_differences(name, cases, got, want):
    (rec, masks), (hrec, hmasks) = got, want
    out = ["%s: field %s" % (name, k) for k in hrec.dtype.names if rec[k].tobytes() != hrec[k].tobytes()]
    if masks.shape != hmasks.shape:
        return out + ["%s: mask shape %s" % (name, masks.shape)]
    diff = masks ^ hmasks
    mine = sorted({"%s[%s]" % (g, s) for g, s, h, i, _ in cases if gb.bit(diff, h, i)})
    other = sum(bin(int(w)).count("1") for w in diff.reshape(-1)) - sum(gb.bit(diff, h, i) for _, _, h, i, _ in cases)
    return out + ["%s: %s" % (name, k) for k in mine] + (["%s: %d bits without a case" % (name, other)] if other else [])


def test_sim3_boundaries_one_call_per_problem(matcher):
    import multi_orb_slam_amd as m
    differing = []
    for (name, W, cases), want in zip(gb.sim3_problems(), gb.sim3_host_answers()):
        got, = matcher.Sim3Ransac([sw.to_problem(m, W)])
        assert matcher.last_sim3() == (1, 0), name
        differing += sim3_differences(name, cases, got, want)
    assert not differing, differing


def test_sim3_boundaries_in_one_batch(matcher):
    """All problems in one call: the first mask word of a problem is then the sum of the earlier problems' hypotheses x words."""
    import multi_orb_slam_amd as m
    probs = gb.sim3_problems()
    assert len(probs) <= m.SIM3_MAX_BATCH
    got = matcher.Sim3Ransac([sw.to_problem(m, W) for _, W, _ in probs])
    assert matcher.last_sim3() == (len(probs), 0)
    differing = []
    for (name, W, cases), g, want in zip(probs, got, gb.sim3_host_answers()):
        differing += sim3_differences(name, cases, g, want)
    assert not differing, differing


# ---- pose --------------------------------------------------------------------------------------------------------------------------------
def pose_differences(name, case, got, want):
    (rec, flags), (hrec, hflags) = got, want
    group, side, edge, _ = case
    out = ["%s [%s / %s]: field %s" % (name, group, side, k) for k in hrec.dtype.names if rec[k].tobytes() != hrec[k].tobytes()]
    bad = np.flatnonzero(flags != hflags)
    if len(bad):
        out.append("%s [%s / %s]: flags of edges %s%s" % (name, group, side, bad[:8].tolist(), " (the case's edge among them)" if edge in bad else ""))
    return out


def test_pose_boundaries_one_call_per_problem(matcher):
    import multi_orb_slam_amd as m
    differing = []
    for (name, P, case), want in zip(gb.pose_problems(), gb.pose_host_answers()):
        got, = matcher.PoseOptimization([pw.to_problem(m, P)])
        assert matcher.last_pose() == (1, 0), name
        differing += pose_differences(name, case, got, want)
    assert not differing, differing


def test_pose_boundaries_in_one_batch(matcher):
    import multi_orb_slam_amd as m
    probs = gb.pose_problems()
    got = matcher.PoseOptimization([pw.to_problem(m, P) for _, P, _ in probs])
    assert matcher.last_pose() == (len(probs), 0)
    differing = []
    for (name, P, case), g, want in zip(probs, got, gb.pose_host_answers()):
        differing += pose_differences(name, case, g, want)
    assert not differing, differing
