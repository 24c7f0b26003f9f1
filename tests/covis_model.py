"""A model of the two counting routines of the LocalMapping / LoopClosing threads, written from the reference's functions and in
their shape -- objects, a dict per point for mObservations / mObservations_cam1, a dict per keyframe for KFcounter -- not from the
library: KeyFrame::UpdateConnections' two counters (src/KeyFrame.cc:486-552) and LocalMapping::KeyFrameCulling's counts and verdict
(src/LocalMapping.cc:966-1038).  The plain arrays of a world (tests/covis_worlds.py) are turned into those objects first."""
import numpy as np

BAD, FAR, LEVEL_MASK = 1, 0x80, 0x1f
COVIS_DTYPE = np.dtype([("keyframe", "<i4"), ("all", "<i4"), ("cam1", "<i4")])


class MapPoint:
    def __init__(self, bad, n_obs):
        self.bad, self.nObs = bool(bad), int(n_obs)
        self.mObservations, self.mObservations_cam1 = {}, {}

    def AddObservation(self, kf, idx):      # src/MapPoint.cc:138-165, without the counter (nObs is mirrored as a value)
        if kf in self.mObservations:
            return
        self.mObservations[kf] = idx
        if idx < kf.N:
            self.mObservations_cam1[kf] = idx


class KeyFrame:
    def __init__(self, mnId, points, levels, far, N):
        self.mnId, self.mvpMapPoints, self.octave, self.far, self.N = mnId, points, levels, far, int(N)


def build(w):
    """The objects of a world: (keyframes, points)."""
    pts = [MapPoint(w["flags"][p] & BAD, w["n_obs"][p]) for p in range(w["n_points"])]
    kfs = []
    for k in range(w["n_kfs"]):
        c = int(w["kf_count"][k])
        row = [pts[s] if s >= 0 else None for s in w["kf_rows"][k, :c].tolist()]
        fb = w["kf_feat"][k]
        kfs.append(KeyFrame(k, row, (fb & LEVEL_MASK).tolist(), ((fb & FAR) != 0).tolist(), w["kf_ncam1"][k]))
    obs, feat = w["obs"], w["obs_feat"]
    for r in range(len(obs)):
        if obs["point"][r] >= 0:
            pts[obs["point"][r]].AddObservation(kfs[obs["keyframe"][r]], int(feat[r]))
    return kfs, pts


def update_connections_counters(pKF):
    """src/KeyFrame.cc:489-552 -> (KFcounter, KFcounter_cam1), dicts keyed by keyframe object."""
    KFcounter, KFcounter_cam1 = {}, {}
    vpMP = list(pKF.mvpMapPoints)
    vpMP_cam1 = [pKF.mvpMapPoints[i] for i in range(min(pKF.N, len(pKF.mvpMapPoints)))]
    for pMP in vpMP:
        if pMP is None:
            continue
        if pMP.bad:
            continue
        observations = dict(pMP.mObservations)
        for kf in observations:
            if kf.mnId == pKF.mnId:
                continue
            KFcounter[kf] = KFcounter.get(kf, 0) + 1
    for pMP in vpMP_cam1:
        if pMP is None:
            continue
        if pMP.bad:
            continue
        observations_cam1 = dict(pMP.mObservations_cam1)
        for kf in observations_cam1:
            if kf.mnId == pKF.mnId:
                continue
            KFcounter_cam1[kf] = KFcounter_cam1.get(kf, 0) + 1
    return KFcounter, KFcounter_cam1


def covisibility(w, kfs_listed, objects=None):
    """-> one COVIS_DTYPE array per listed keyframe: the entries of KFcounter in ascending slot, cam1 from KFcounter_cam1 (0 if absent)."""
    kfs, _ = objects or build(w)
    out = []
    for k in np.asarray(kfs_listed).tolist():
        a, c = update_connections_counters(kfs[k])
        assert set(c) <= set(a)                       # (an observation of camera 1 is an observation)
        e = np.zeros(len(a), COVIS_DTYPE)
        for i, kf in enumerate(sorted(a, key=lambda x: x.mnId)):
            e[i] = (kf.mnId, a[kf], c.get(kf, 0))
        out.append(e)
    return out


def culling_counts_of(pKF, mono):
    """src/LocalMapping.cc:983-1032 for one keyframe -> (nMPs, nRedundantObservations)."""
    vpMapPoints = pKF.mvpMapPoints
    nObs = 3
    thObs = nObs
    nRedundantObservations = 0
    nMPs = 0
    for i in range(len(vpMapPoints)):
        pMP = vpMapPoints[i]
        if pMP is not None:
            if not pMP.bad:
                if not mono:
                    if pKF.far[i]:                    # mvDepth_total[i] > mThDepth || mvDepth_total[i] < 0, evaluated by the host
                        continue
                nMPs += 1
                if pMP.nObs > thObs:
                    scaleLevel = pKF.octave[i]
                    observations = dict(pMP.mObservations)
                    nObs = 0
                    for pKFi, idx in observations.items():
                        if pKFi is pKF:
                            continue
                        scaleLeveli = pKFi.octave[idx]
                        if scaleLeveli <= scaleLevel + 1:
                            nObs += 1
                            if nObs >= thObs:
                                break
                    if nObs >= thObs:
                        nRedundantObservations += 1
    return nMPs, nRedundantObservations


def culling_counts(w, kfs_listed, mono=False, objects=None):
    kfs, _ = objects or build(w)
    return np.array([culling_counts_of(kfs[k], mono) for k in np.asarray(kfs_listed).tolist()], np.int32).reshape(-1, 2)


def culled(nRedundantObservations, nMPs):
    """src/LocalMapping.cc:1035: an int against a double product."""
    return float(nRedundantObservations) > 0.90 * float(nMPs)
