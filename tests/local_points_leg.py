"""Run as a child process with MORB_HOST_RESOLVE=1 (read once, in orbm_create): orbm_search_local_points through the exact host
fallback -- queries rebuilt on the host from the table's mirror, candidates from the device, the sequential resolve on the host
-- on one generated world, held against the model + oracle byte for byte.  Prints `local_points_leg ok ...`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import multi_orb_slam_amd as m
import oracle
import frustum_model as fm
import frustum_worlds as fw

case = fw.CASES[int(sys.argv[1])]
w = fw.make_world(*case)
rng = np.random.default_rng(99)
skip = (rng.random(case[0]) < 0.1).astype(np.uint8)
occ = (rng.random(len(w["fr"]["un_x"])) < 0.1).astype(np.uint8)
mt = m.Matcher(0.8, True)
F = mt.frame(m.FrameData(**w["fr"])); OF = oracle.FrameData(**w["fr"])
with m.LocalPoints(mt, case[0]) as pts:
    pts.write(0, w["points"])
    for sk, oc in ((None, None), (skip, occ)):
        e_ntm, e_nm, e_mo, e_track, _ = fm.expected_search(OF, w["points"], w["view"], sk, oc, 0.8, 100)
        ntm, nm, mo, track = mt.SearchLocalPoints(F, pts, w["view"].native(), sk, oc)
        assert mt.last_resolve()[0] == -1, mt.last_resolve()       # the host path was taken
        assert (ntm, nm) == (e_ntm, e_nm) and e_nm > 0, (ntm, nm, e_ntm, e_nm)
        assert np.array_equal(mo, e_mo) and track.tobytes() == e_track.tobytes()
F.close(); mt.close()
print("local_points_leg ok: %d points, %d in view, %d matches through the host fallback" % (case[0], e_ntm, e_nm))
