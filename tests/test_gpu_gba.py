"""GPU parity of the global bundle adjustment on the device (orbm_bundle_adjust: the local BA's kernels, the reduced system over the
block pairs that exist, the blocked LDL^T across workgroups) with the library's host routine in DEVICE order -- byte for byte: every
estimate, every float handed to SetPose / SetWorldPos, the round record, the poll count -- and of the device solver alone
(orbm_ba_ldlt_device) with the sequential routine that defines it (orbm_ba_ldlt), at sizes around the panel width."""
import ctypes as C
import numpy as np
import pytest

import gba_worlds as gw
import lba_worlds as lw

pytestmark = pytest.mark.gpu
DEVICE_WORLDS = ["f1_p150_mixed", "f10_p150_mixed_wrong10", "f11_p150_stereo", "f64_p400_mixed_wrong10", "f65_p400_mixed_wrong10",
                 "f96_p600_mono_wrong10"]
gw.WORLDS.setdefault("f1_p150_mixed", (1, 150, 111, "mixed", 0.0, 5, True))


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def device_and_host(mt, W, iterations, robust, stop=None, path=0):
    import multi_orb_slam_amd as m
    P = gw.to_problem(m, W)
    dev = mt.bundle_adjust(P, iterations, robust, stop=stop)
    last = mt.last_bundle_adjust()
    hst = m.bundle_adjust_host(P, iterations, robust, m.POSE_ORDER_DEVICE, stop=stop)
    assert dev.same_bytes(hst) is None, (dev.same_bytes(hst), dev.round, hst.round)
    assert last[0] == path and last[3] == hst.polls and last[7] == 0
    if path == 0:
        # one synchronisation per Levenberg trial, plus: the optimisation begun, a stop inside a trial loop, the last
        assert last[2] <= int(hst.round["trials"][0]) + 3 and last[1] > 0
        na = hst.active_poses
        assert last[5] == na * (na + 1) // 2 and na <= last[4] <= last[5] and last[6] == (6 * na + m.BA_PANEL - 1) // m.BA_PANEL
    else:
        assert last[1] == 0 and last[2] == 0
    return dev, last


# ---- the solver alone --------------------------------------------------------------------------------------------------------------------
def random_spd(n, seed):
    rng = np.random.RandomState(seed)
    A = rng.uniform(-1, 1, (n, n))
    return A @ A.T + n * np.eye(n), rng.uniform(-1, 1, n)


def integer_ldl(n, seed, zero_at=None):
    """H = L D L^T of small integers: L unit lower triangular with entries -1 / 0 / 1 (one in ten), D from 1, 2, 3, -1, -2 -- indefinite,
    no pivot zero -- or 0 at zero_at.  Every quantity of the factorisation is a small integer, so it is exact in double and pivot
    zero_at is an EXACT zero, reached after the columns before it factorised."""
    rng = np.random.RandomState(seed)
    L = np.tril(rng.choice([-1.0, 0.0, 1.0], size=(n, n), p=[0.05, 0.9, 0.05]), -1) + np.eye(n)
    D = rng.choice([1.0, 2.0, 3.0, -1.0, -2.0], size=n)
    if zero_at is not None:
        D[zero_at] = 0.0
    return (L * D) @ L.T, rng.randint(-4, 5, n).astype(np.float64)


def solve_raw(mt, H, b):
    """orbm_ba_ldlt_device on x prefilled with a sentinel -> (return value, x)."""
    from multi_orb_slam_amd import _lib
    H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.full(len(b), -77.25)
    rc = _lib.lib().orbm_ba_ldlt_device(mt._h, len(b), _lib.ptr(H), _lib.ptr(b), _lib.ptr(x))
    return rc, x


def sizes():
    import multi_orb_slam_amd as m
    w = m.BA_PANEL
    return [1, 6, w - 4, w, w + 1, 2 * w, 6 * 65, 1026]


@pytest.mark.parametrize("k", range(8))
def test_the_device_solver_equals_the_sequential_routine(matcher, k):
    import multi_orb_slam_amd as m
    n = sizes()[k]
    for H, b in (integer_ldl(n, 500 + n), random_spd(n, 400 + n)):
        want = m.ba_ldlt(H, b)
        rc, got = solve_raw(matcher, H, b)
        assert want is not None and rc == 1 and got.tobytes() == want.tobytes(), (n, int((got != want).sum()))
    assert np.abs(H @ got - b).max() <= 1e-12 * n                  # (the definite system is well conditioned: it is solved, too)


@pytest.mark.parametrize("k", range(8))
def test_a_zero_pivot_anywhere_returns_0_and_leaves_x(matcher, k):
    import multi_orb_slam_amd as m
    n, w = sizes()[k], m.BA_PANEL
    places = sorted({p for p in (0, min(5, n - 1), w - 1, w, w + 1, n - 1) if p < n})      # the first panel, across the boundary, the last row
    for z in places:
        H, b = integer_ldl(n, 600 + n + z, zero_at=z)
        assert m.ba_ldlt(H, b) is None
        rc, x = solve_raw(matcher, H, b)
        assert rc == 0 and (x == -77.25).all(), (n, z, rc)
    H, b = random_spd(n, 700 + n)
    H[n - 1, n - 1] = np.nan                                                                # a non-finite pivot in the last row
    rc, x = solve_raw(matcher, H, b)
    assert m.ba_ldlt(H, b) is None and rc == 0 and (x == -77.25).all()
    H, b = random_spd(n, 800 + n)                                                            # ... and the next call is not affected
    rc, x = solve_raw(matcher, H, b)
    assert rc == 1 and x.tobytes() == m.ba_ldlt(H, b).tobytes()


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [(10, False), (20, True)], ids=["10-plain", "20-robust"])
@pytest.mark.parametrize("name", DEVICE_WORLDS)
def test_device_equals_the_host_routine_in_device_order(matcher, name, mode):
    R, last = device_and_host(matcher, gw.world(name), *mode)
    f = gw.WORLDS[name][0]
    assert R.optimised == 1 and R.active_poses == f and R.round["iterations"][0] >= 1
    if f >= 10:
        assert last[4] < last[5], "a trajectory: most pose pairs share no point"


def test_a_65_pose_world_runs_on_the_device_and_the_local_ba_still_takes_its_host_path(matcher):
    import multi_orb_slam_amd as m
    W = lw.world("f65_x3_p150_mixed")
    assert W["n_free"] == m.LBA_MAX_FREE + 1
    device_and_host(matcher, W, 10, False, path=0)
    matcher.local_ba(lw.to_problem(m, W))
    assert matcher.last_local_ba()[0] == 1


def test_every_block_pair_is_computed_where_every_keyframe_sees_every_point(matcher):
    R, last = device_and_host(matcher, gw.world("f12_p150_dense_mixed"), 10, True)
    assert R.active_poses == 12 and last[4] == last[5] == 78


@pytest.mark.parametrize("name", list(gw.hand_cases()))
def test_hand_built_cases(matcher, name):
    import multi_orb_slam_amd as m
    bad_pose = 12                                    # its pivot is row 72: beyond the first panel
    assert 6 * bad_pose >= m.BA_PANEL
    W, robust, expect = gw.hand_cases(16, bad_pose)[name]
    R, last = device_and_host(matcher, W, 10, robust, stop=10 ** 9, path=2 if name == "no_edges" else 0)
    assert expect(R), name
    if name in ("zero_pivot", "non_finite_pivot_at_a_pose"):
        assert np.array_equal(R.point_f, W["points"])                      # every solve failed: nothing moved


@pytest.mark.parametrize("name", list(gw.stop_cases()))
def test_stop_cases(matcher, name):
    W, iterations, robust, n, _, polls = gw.stop_cases()[name]
    R, _ = device_and_host(matcher, W, iterations, robust, stop=n)
    assert R.polls == polls


def test_the_call_made_twice_gives_the_same_result(matcher):
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    W = gw.world("f65_p400_mixed_wrong10")
    a, _ = device_and_host(matcher, W, 10, True)
    device_and_host(matcher, gw.world("f10_p150_mixed_wrong10"), 10, True)       # (the buffers are reused by a smaller call in between)
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)                       # ... and by an unrelated search
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(w["points"])) as pts:
        pts.write(0, w["points"])
        _, nmatches, _, _ = matcher.SearchLocalPoints(F, pts, w["view"].native())
        assert nmatches > 100
        b, _ = device_and_host(matcher, W, 10, True)
    F.close()
    assert a.same_bytes(b) is None


def test_a_problem_past_the_cap_or_without_an_active_free_pose_reports_the_host_path(matcher):
    import multi_orb_slam_amd as m
    W = gw.make_world(m.BA_MAX_FREE + 1, 40, 120, "mixed", 0.0, 4, True, "near")          # few points: few poses are active
    R, _ = device_and_host(matcher, W, 5, True, path=1)
    assert 0 < R.active_poses < 200
    W = gw.make_world(0, 25, 121, "stereo", 0.0, 3, True, "near", n_fixed=3)             # no free pose at all
    R, _ = device_and_host(matcher, W, 5, True, path=2)
    assert R.optimised == 1 and R.active_poses == 0 and R.round["iterations"][0] >= 1
