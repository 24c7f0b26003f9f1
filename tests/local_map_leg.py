"""Child process of tests/test_gpu_local_map.py, started with MORB_HOST_RESOLVE=1 (read in orbm_create): the resident map's three calls
through their exact host route -- the votes and the point list from the host routines over the mirror, the search through the host
restatement of the frustum test and host_resolve with the skip flags rebuilt from the mirror -- against the same inputs through the
plain-array routines and the existing search over a table in list order.  Prints 'local_map_leg ok'."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import multi_orb_slam_amd as m  # noqa: E402
import frustum_worlds as fw  # noqa: E402
import localmap_worlds as lw  # noqa: E402


def main():
    assert os.environ.get("MORB_HOST_RESOLVE") == "1"
    n = 2000
    w = fw.make_world(n, [1000, 500], 640, 480, 2, 3.0)
    nf = len(w["fr"]["un_x"])
    rng = np.random.default_rng(12)
    slots = rng.permutation(4 * n)[:n].astype(np.int32)
    flags = (rng.random(n) < 0.05).astype(np.uint8)
    all_flags = np.zeros(4 * n, np.uint8); all_flags[slots] = flags
    mt = m.Matcher(0.8, True)
    F = mt.frame(m.FrameData(**w["fr"]))
    view = w["view"].native()
    with m.ResidentMap(mt, 3, 4 * n, 3 * n, 1200) as rm, m.LocalPoints(mt, n) as table:
        rm.write_points(slots, w["points"], flags)
        shuffled = slots[rng.permutation(n)]
        rows = np.full((3, 1200), -1, np.int32); count = np.array([1000, 1200, 700], np.int32)
        rows[0, :1000] = shuffled[:1000]; rows[1, :1000] = shuffled[1000:]; rows[1, 1000:1200] = shuffled[:200]; rows[2, :700] = shuffled[600:1300]
        obs = np.zeros(int(count.sum()), lw.OBS_DTYPE)
        obs["point"] = np.concatenate([rows[k, :count[k]] for k in range(3)]); obs["keyframe"] = np.repeat(np.arange(3), count)
        obs = obs[np.unique(obs, return_index=True)[1]]                       # one record per (point, keyframe)
        for k in range(3):
            rm.write_keyframe(k, rows[k, :count[k]])
        rm.write_observations(np.arange(len(obs)), obs)
        fp = np.where(rng.random(nf) < 0.1, slots[rng.integers(0, n, nf)], -1).astype(np.int32)
        votes = rm.vote(fp)
        assert mt.last_local_map(rm)[0] == 0                                # the host route ran
        assert np.array_equal(votes, m.local_map_vote_host(obs, all_flags, fp, 3)) and votes.sum() > 0
        lst = rm.local_points([2, 0, 1])
        assert np.array_equal(lst, m.local_map_points_host(rows, count, all_flags, [2, 0, 1])) and len(lst) == int((flags == 0).sum())
        row_of_slot = np.full(4 * n, -1, np.int64); row_of_slot[slots] = np.arange(n)
        table.write(0, w["points"][row_of_slot[lst]])
        seen = lst[rng.permutation(len(lst))[:150]]
        good = fp[fp >= 0]; good = good[all_flags[good] == 0]
        skip = (np.isin(lst, good) | np.isin(lst, seen)).astype(np.uint8)
        occ = (fp >= 0).astype(np.uint8)
        exp = mt.SearchLocalPoints(F, table, view, skip, occ, n=len(lst))
        got = rm.search(F, view, fp, seen, occ, n_list=len(lst))
        assert got[:2] == exp[:2] and got[1] > 20 and skip.sum() > 100
        assert got[2].tobytes() == exp[2].tobytes() and got[3].tobytes() == exp[3].tobytes()
    F.close(); mt.close()
    print("local_map_leg ok")


if __name__ == "__main__":
    main()
