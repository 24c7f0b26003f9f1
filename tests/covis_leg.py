"""Child process of tests/test_gpu_covis.py, started with MORB_HOST_RESOLVE=1 (read in orbm_create): orbm_map_covisibility and
orbm_map_culling_counts through their host route -- the host routines over the map's mirror -- against the same routines on the
world's plain arrays and against the model.  Prints 'covis_leg ok'."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import multi_orb_slam_amd as m  # noqa: E402
from multi_orb_slam_amd import _lib  # noqa: E402
import covis_model as cm  # noqa: E402
import covis_worlds as cw  # noqa: E402


def main():
    assert os.environ.get("MORB_HOST_RESOLVE") == "1"
    w = cw.make_world(21, 50, 600, 48, 4000)
    listed = np.random.default_rng(21).permutation(50)[:20].astype(np.int32)
    mt = m.Matcher(0.8, True)
    with cw.to_resident(m, mt, w, kf_capacity=64, obs_capacity=len(w["obs"]) + 50) as rm:
        e_cov, e_cull = cw.host(m, w, listed)
        assert cw.same_lists(e_cov, cm.covisibility(w, listed)) and np.array_equal(e_cull, cm.culling_counts(w, listed))
        for _ in range(2):
            assert cw.same_lists(rm.covisibility(listed), e_cov)
            assert rm.last_covisibility() == (0, 0, len(w["obs"]), len(listed))     # the host route ran, no index was built
            assert np.array_equal(rm.culling_counts(listed), e_cull)
            assert np.array_equal(rm.culling_counts(listed, mono=True), cw.host(m, w, listed, True)[1])
        total = sum(len(e) for e in e_cov)
        try:
            rm.covisibility(listed, entries_cap=total - 1)
            raise AssertionError("no capacity error")
        except m.OrbError as e:
            assert e.code == _lib.ORB_E_CAPACITY and str(total) in str(e)
        assert total > 50 and e_cull[:, 1].sum() > 0
    mt.close()
    print("covis_leg ok")


if __name__ == "__main__":
    main()
