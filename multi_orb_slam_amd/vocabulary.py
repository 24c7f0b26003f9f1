"""ctypes mirror of include/orbv.h: vocabulary-tree transform (DBoW2) and the BoW-gated searches of ORBmatcher."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import BowSide, Triangulation, TriGeometry, check, ptr

# orbv_tri_out: the record of one pair of the triangulation stage
TRI_OUT_DTYPE = np.dtype([("x3D", np.float32, 3), ("outcome", np.int32), ("path", np.int32)])
TRI_NONE, TRI_ACCEPTED, TRI_CAM_OFF, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_Z1, TRI_Z2, TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE = range(11)
TRI_PATH_NONE, TRI_PATH_SVD, TRI_PATH_UNPROJECT1, TRI_PATH_UNPROJECT2 = range(4)


class FeatureVector:
    """DBoW2::FeatureVector as CSR arrays: node ids ascending, feature indices per node in push_back order."""

    def __init__(self, node_id, node_start, items):
        self.node_id = np.ascontiguousarray(node_id, np.uint32)
        self.node_start = np.ascontiguousarray(node_start, np.int32)
        self.items = np.ascontiguousarray(items, np.uint32)

    def as_dict(self):
        return {int(k): self.items[self.node_start[i]:self.node_start[i + 1]].tolist() for i, k in enumerate(self.node_id)}


class Vocabulary:
    def __init__(self, parent=None, is_leaf=None, desc=None, weight=None, L=None, device=0, path=None):
        self._h = C.c_void_p()
        if path is not None:
            check(_lib.lib().orbv_load_text(str(path).encode(), device, C.byref(self._h)))
        else:
            parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
            desc = np.ascontiguousarray(desc, np.uint8); weight = np.ascontiguousarray(weight, np.float64)
            check(_lib.lib().orbv_create(len(parent), int(L), ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight), device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbv_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def stream(self):
        return _lib.lib().orbv_stream(self._h)

    def info(self):
        v = [C.c_int() for _ in range(4)]
        check(_lib.lib().orbv_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_nodes", "n_words", "k", "L"), (x.value for x in v)))

    def transform(self, features, levelsup=4):
        """-> (word_id, node_id, weight) per feature."""
        f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(f)
        w, nd, wt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        check(_lib.lib().orbv_transform(self._h, ptr(f), n, levelsup, ptr(w), ptr(nd), ptr(wt)))
        return w, nd, wt

    def transform_device(self, d_features, n, levelsup, d_word, d_node, stream):
        check(_lib.lib().orbv_transform_device(self._h, C.c_void_p(d_features), n, levelsup, C.c_void_p(d_word), C.c_void_p(d_node),
                                               C.c_void_p(stream) if stream else None))

    def bow_vectors(self, features, levelsup=4):
        """transform(features, BowVector, FeatureVector, levelsup) -> ((word ids, values), FeatureVector)."""
        f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(f)
        bid, bval = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        fn, fs, fi = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(), C.c_int()
        check(_lib.lib().orbv_bow_vectors(self._h, ptr(f), n, levelsup, ptr(bid), ptr(bval), C.byref(nw), ptr(fn), ptr(fs), ptr(fi), C.byref(nn)))
        return (bid[:nw.value].copy(), bval[:nw.value].copy()), FeatureVector(fn[:nn.value], fs[:nn.value + 1], fi[:fs[nn.value]])


def score_l1(a, b):
    """L1Scoring::score of two (ids, values) sparse vectors."""
    ia, va = np.ascontiguousarray(a[0], np.uint32), np.ascontiguousarray(a[1], np.float64)
    ib, vb = np.ascontiguousarray(b[0], np.uint32), np.ascontiguousarray(b[1], np.float64)
    return _lib.lib().orbv_score_l1(ptr(ia), ptr(va), len(ia), ptr(ib), ptr(vb), len(ib))


def _bow(b):
    return np.ascontiguousarray(b[0], np.uint32), np.ascontiguousarray(b[1], np.float64)


DB_FORM_LDS, DB_FORM_GLOBAL = 1, 2     # ORBV_DB_FORM_* of include/orb_debug.h


class KeyFrameDatabase:
    """Resident keyframe database (orbv_database): BowVectors stay in HBM, a query returns the reference's lKFsSharingWords."""

    def __init__(self, n_words, device=0):
        self._h = C.c_void_p()
        check(_lib.lib().orbv_db_create(int(n_words), device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbv_db_destroy(self._h)
            self._h = None

    __del__ = close

    def add(self, key, bow):
        ids, vals = _bow(bow)
        check(_lib.lib().orbv_db_add(self._h, int(key), ptr(ids), ptr(vals), len(ids)))

    def erase(self, key):
        check(_lib.lib().orbv_db_erase(self._h, int(key)))

    def clear(self):
        check(_lib.lib().orbv_db_clear(self._h))

    def __len__(self):
        return _lib.lib().orbv_db_count(self._h)

    def query(self, bows, capacity=None):
        """-> per query (keys, common, score) of the entries sharing a word with it, in the order of the reference's list."""
        qs = [_bow(b) for b in bows]
        Q = len(qs)
        cap = len(self) if capacity is None else int(capacity)
        pid = (C.c_void_p * max(Q, 1))(*[a[0].ctypes.data for a in qs]); pval = (C.c_void_p * max(Q, 1))(*[a[1].ctypes.data for a in qs])
        n = np.array([len(a[0]) for a in qs] + [0], np.int32)
        keys, common = np.zeros(max(Q * cap, 1), np.uint64), np.zeros(max(Q * cap, 1), np.int32)
        score, hits = np.zeros(max(Q * cap, 1), np.float64), np.zeros(max(Q, 1), np.int32)
        check(_lib.lib().orbv_db_query(self._h, Q, pid, pval, ptr(n), cap, ptr(keys), ptr(common), ptr(score), ptr(hits)))
        return [(keys[q * cap:q * cap + hits[q]].copy(), common[q * cap:q * cap + hits[q]].copy(), score[q * cap:q * cap + hits[q]].copy())
                for q in range(Q)]

    def last_query(self):
        """(form: DB_FORM_LDS or DB_FORM_GLOBAL, entries per workgroup, workgroups per query, queries) of the last kernel launch behind
        query / score (orbv_debug_last_db_query)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbv_debug_last_db_query(self._h, out))
        return tuple(out)

    def score(self, bow, keys):
        """L1 score of `bow` against the named entries."""
        ids, vals = _bow(bow)
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros(max(len(keys), 1), np.float64)
        check(_lib.lib().orbv_db_score(self._h, ptr(ids), ptr(vals), len(ids), ptr(keys), len(keys), ptr(out)))
        return out[:len(keys)]


def cos_stereo(mb, depth):
    """cos(2*atan2(mb/2, depth)) per feature with the float overloads of the reference's statement (orbv_cos_stereo, host libm)."""
    d = np.ascontiguousarray(depth, np.float32)
    out = np.zeros(len(d), np.float32)
    check(_lib.lib().orbv_cos_stereo(float(np.float32(mb)), ptr(d), len(d), ptr(out)))
    return out


class TriKeyframe:
    """One keyframe as the triangulation stage reads it (orbv_tri_keyframe); keeps the arrays alive.  Tcw: (2, 3, 4) per camera
    [R|t]; centre: (2, 3); Twc: (3, 4); the per-feature arrays may be left out for the resident calls."""

    FEATURE_ARRAYS = (("x", np.float32), ("y", np.float32), ("xd", np.float32), ("yd", np.float32), ("octave", np.int32),
                      ("uright", np.float32), ("depth", np.float32), ("cos_stereo", np.float32), ("cam_of", np.int32))

    def __init__(self, Tcw, centre, Twc, Rcam12, tcam12, fx, fy, cx, cy, invfx, invfy, mbf, scale_factors, level_sigma2, n_cam1, n=None,
                 **arrays):
        f32 = lambda a, shape: np.ascontiguousarray(a, np.float32).reshape(shape)
        self.Tcw, self.centre, self.Twc = f32(Tcw, (2, 12)), f32(centre, (2, 3)), f32(Twc, 12)
        self.Rcam12, self.tcam12 = f32(Rcam12, 9), f32(tcam12, 3)
        self.scalars = [float(np.float32(v)) for v in (fx, fy, cx, cy, invfx, invfy, mbf)]
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        self.n_levels = len(self.scale_factors)     # (set n_levels afterwards to describe a table shorter than the array)
        self.n_cam1 = int(n_cam1)
        for name, dt in self.FEATURE_ARRAYS:
            a = arrays.pop(name, None)
            setattr(self, name, None if a is None else np.ascontiguousarray(a, dt))
        assert not arrays, "unknown arrays: %s" % sorted(arrays)
        self.n = int(n) if n is not None else (len(self.x) if self.x is not None else 0)

    def c(self):
        k = _lib.TriKeyframe()
        for cam in range(2):
            for j in range(12):
                k.Tcw[cam][j] = float(self.Tcw[cam, j])
            for j in range(3):
                k.centre[cam][j] = float(self.centre[cam, j])
        for j in range(12):
            k.Twc[j] = float(self.Twc[j])
        for j in range(9):
            k.Rcam12[j] = float(self.Rcam12[j])
        for j in range(3):
            k.tcam12[j] = float(self.tcam12[j])
        k.fx, k.fy, k.cx, k.cy, k.invfx, k.invfy, k.mbf = self.scalars
        k.n_levels = self.n_levels; k.scale_factors = self.scale_factors.ctypes.data; k.level_sigma2 = self.level_sigma2.ctypes.data
        k.n = self.n; k.n_cam1 = self.n_cam1
        for name, _ in self.FEATURE_ARRAYS:
            a = getattr(self, name)
            setattr(k, name, None if a is None else a.ctypes.data)
        return k


def _pairs(pairs):
    p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return p, np.zeros(max(len(p), 1), TRI_OUT_DTYPE)


def triangulate_pairs_host(kf1, kf2, cam_enabled, pairs, ratio_factor):
    """The pair loop of LocalMapping::CreateNewMapPoints on the host (orbv_triangulate_pairs_host; needs no device) -> TRI_OUT_DTYPE records."""
    p, out = _pairs(pairs)
    c1, c2 = kf1.c(), kf2.c()
    en = np.ascontiguousarray(cam_enabled, np.uint8)
    check(_lib.lib().orbv_triangulate_pairs_host(C.byref(c1), C.byref(c2), ptr(en), ptr(p), len(p), float(np.float32(ratio_factor)), ptr(out)))
    return out[:len(p)]


class Side:
    """One frame / keyframe for the BoW searches (orbv_side); keeps the arrays alive."""

    def __init__(self, desc, angle, fv, flags=None, x=None, y=None, octave=None, cam_of=None):
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.n = len(self.desc)
        self.angle = np.ascontiguousarray(angle, np.float32)
        self.fv = fv
        self.flags = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        self.x = None if x is None else np.ascontiguousarray(x, np.float32)
        self.y = None if y is None else np.ascontiguousarray(y, np.float32)
        self.octave = None if octave is None else np.ascontiguousarray(octave, np.int32)
        self.cam_of = None if cam_of is None else np.ascontiguousarray(cam_of, np.int32)

    def c(self):
        p = lambda a: None if a is None else a.ctypes.data
        return BowSide(self.n, p(self.desc), p(self.angle), p(self.flags), len(self.fv.node_id), p(self.fv.node_id), p(self.fv.node_start),
                       p(self.fv.items), p(self.x), p(self.y), p(self.octave), p(self.cam_of))


class BowSearch:
    """Stream + scratch of the BoW-gated searches (orbv_workspace)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(_lib.lib().orbv_workspace_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbv_workspace_destroy(self._h)
            self._h = None

    __del__ = close

    def search_by_bow(self, a, b, mode, th_low=50, nnratio=0.7, check_orientation=True):
        """mode 0: SearchByBoW(KF a, Frame b) -> match per feature of b; mode 1: (KF a, KF b) -> match per feature of a."""
        n_out = b.n if mode == 0 else a.n
        match = np.full(max(n_out, 1), -1, np.int32); nm = C.c_int()
        ca, cb = a.c(), b.c()
        check(_lib.lib().orbv_search_by_bow(self._h, C.byref(ca), C.byref(cb), mode, th_low, nnratio, int(check_orientation), ptr(match), C.byref(nm)))
        return nm.value, match[:n_out]

    def last_join(self):
        """(waves per node, largest node of b, candidates staged in LDS, mode) of the last search enqueued here (orbv_debug_last_join)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbv_debug_last_join(self._h, out))
        return tuple(out)

    def keyframe_from_device(self, vocabulary, feats, levelsup=4, triangulation=True):
        """Keyframe built entirely on the device from a front end's resident frame (feats = NativeFrontEnd.export_features())."""
        from ._lib import DeviceSide
        s = DeviceSide()
        s.n = feats.n_total; s.d_desc = feats.d_desc; s.d_angle = feats.d_angle; s.d_uright = feats.d_uright
        if triangulation:
            s.d_x = feats.d_un_x; s.d_y = feats.d_un_y; s.d_octave = feats.d_octave
        s.n_cams = feats.n_cams
        acc = 0
        for c in range(feats.n_cams):
            s.cam_start[c] = acc; acc += feats.counts[c]
        s.cam_start[feats.n_cams] = acc
        k = Keyframe.__new__(Keyframe)
        k._h = C.c_void_p(); k.n = feats.n_total; k._search = self
        check(_lib.lib().orbv_keyframe_from_device(self._h, vocabulary._h, C.byref(s), levelsup, C.c_void_p(feats.stream) if feats.stream else None, C.byref(k._h)))
        return k

    def last_keyframe_build(self):
        """(bins, chunks of 1024 bins, FeatureVector nodes, largest node, items) of the last keyframe_from_device here
        (orbv_debug_last_keyframe_build); all zero after a refused one."""
        out = (C.c_int * 5)()
        check(_lib.lib().orbv_debug_last_keyframe_build(self._h, out))
        return tuple(out)

    def keyframe_download(self, k):
        """-> (word_id, node_of_feature, FeatureVector) of a device-built keyframe."""
        n = k.n
        w, nd = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        fn, fs, fi = np.zeros(4100, np.uint32), np.zeros(4101, np.int32), np.zeros(max(n, 1), np.uint32)
        nn = C.c_int()
        check(_lib.lib().orbv_keyframe_download(self._h, k._h, ptr(w), ptr(nd), ptr(fn), ptr(fs), ptr(fi), C.byref(nn)))
        return w[:n], nd[:n], FeatureVector(fn[:nn.value], fs[:nn.value + 1], fi[:fs[nn.value]])

    def keyframe(self, side):
        """Upload a Side once (orbv_keyframe_create); pass the result wherever a Side is accepted."""
        return Keyframe(self, side)

    @staticmethod
    def _flags(f):
        return None if f is None else np.ascontiguousarray(f, np.uint8)

    def search_by_bow_resident(self, a, b, mode, flags_a=None, flags_b=None, th_low=50, nnratio=0.7, check_orientation=True):
        n_out = b.n if mode == 0 else a.n
        match = np.full(max(n_out, 1), -1, np.int32); nm = C.c_int()
        fa, fb = self._flags(flags_a), self._flags(flags_b)
        check(_lib.lib().orbv_search_by_bow_resident(self._h, a._h, None if fa is None else ptr(fa), b._h, None if fb is None else ptr(fb), mode,
                                                     th_low, nnratio, int(check_orientation), ptr(match), C.byref(nm)))
        return nm.value, match[:n_out]

    def search_for_triangulation_resident(self, a, b, F12, ex, ey, scale_factors, level_sigma2, flags_a=None, flags_b=None, th_low=50,
                                          check_orientation=True):
        T, keep = self._tri(F12, ex, ey, scale_factors, level_sigma2)
        match = np.full(max(a.n, 1), -1, np.int32); nm = C.c_int()
        fa, fb = self._flags(flags_a), self._flags(flags_b)
        check(_lib.lib().orbv_search_for_triangulation_resident(self._h, a._h, None if fa is None else ptr(fa), b._h, None if fb is None else ptr(fb),
                                                                C.byref(T), th_low, int(check_orientation), ptr(match), C.byref(nm)))
        return nm.value, match[:a.n]

    def triangulate_pairs(self, kf1, kf2, cam_enabled, pairs, ratio_factor):
        """triangulate_pairs_host on the device: one lane per pair (orbv_triangulate_pairs)."""
        p, out = _pairs(pairs)
        c1, c2 = kf1.c(), kf2.c()
        en = np.ascontiguousarray(cam_enabled, np.uint8)
        check(_lib.lib().orbv_triangulate_pairs(self._h, C.byref(c1), C.byref(c2), ptr(en), ptr(p), len(p), float(np.float32(ratio_factor)), ptr(out)))
        return out[:len(p)]

    def create_new_points_resident(self, a, b, F12, ex, ey, scale_factors, level_sigma2, kf1, kf2, cam_enabled, ratio_factor, flags_a=None,
                                   flags_b=None, th_low=50, check_orientation=True):
        """search_for_triangulation_resident and the triangulation of its pairs in one call, one synchronisation
        (orbv_create_new_points_resident) -> (match per feature of a, TRI_OUT_DTYPE record per feature of a, accepted)."""
        T, keep = self._tri(F12, ex, ey, scale_factors, level_sigma2)
        G = TriGeometry()
        G.kf1, G.kf2 = kf1.c(), kf2.c()
        G.cam_enabled[0], G.cam_enabled[1] = int(bool(cam_enabled[0])), int(bool(cam_enabled[1]))
        G.ratio_factor = float(np.float32(ratio_factor))
        match = np.full(max(a.n, 1), -1, np.int32); out = np.zeros(max(a.n, 1), TRI_OUT_DTYPE); acc = C.c_int()
        fa, fb = self._flags(flags_a), self._flags(flags_b)
        check(_lib.lib().orbv_create_new_points_resident(self._h, a._h, None if fa is None else ptr(fa), b._h, None if fb is None else ptr(fb),
                                                         C.byref(T), C.byref(G), th_low, int(check_orientation), ptr(match), ptr(out), C.byref(acc)))
        return match[:a.n], out[:a.n], acc.value

    def create_new_points_keyframe(self, a, rounds, flags_a=None, th_low=50, check_orientation=True):
        """Every neighbour of keyframe `a` in one enqueue with one synchronisation (orbv_create_new_points_keyframe): round k is
        create_new_points_resident against rounds[k] (NewPointsRound), and a feature of `a` whose pair was accepted leaves the searches of
        the rounds behind it -> (match[K, n], TRI_OUT_DTYPE records[K, n], n_matches[K], n_accepted[K])."""
        K, n = len(rounds), a.n
        R = (_lib.NewPointsRound * max(K, 1))()
        keep = []
        for k, r in enumerate(rounds):
            T, kp = self._tri(r.F12, r.ex, r.ey, r.scale_factors, r.level_sigma2)
            fb = self._flags(r.flags_b)
            keep.append((kp, fb))
            R[k].b = r.b._h; R[k].flags_b = None if fb is None else fb.ctypes.data; R[k].t = T
            R[k].geometry.kf1, R[k].geometry.kf2 = r.kf1.c(), r.kf2.c()
            R[k].geometry.cam_enabled[0], R[k].geometry.cam_enabled[1] = int(bool(r.cam_enabled[0])), int(bool(r.cam_enabled[1]))
            R[k].geometry.ratio_factor = float(np.float32(r.ratio_factor))
        match = np.full(max(K * n, 1), -1, np.int32); out = np.zeros(max(K * n, 1), TRI_OUT_DTYPE)
        nm = np.zeros(max(K, 1), np.int32); acc = np.zeros(max(K, 1), np.int32)
        fa = self._flags(flags_a)
        check(_lib.lib().orbv_create_new_points_keyframe(self._h, a._h, None if fa is None else ptr(fa), R, K, th_low, int(check_orientation),
                                                         ptr(match), ptr(out), ptr(nm), ptr(acc)))
        return match[:K * n].reshape(K, n), out[:K * n].reshape(K, n), nm[:K], acc[:K]

    def last_keyframe_call(self):
        """(rounds given, rounds enqueued, kernel launches, stream synchronisations) of the last create_new_points_keyframe here
        (orbv_debug_last_keyframe_call)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbv_debug_last_keyframe_call(self._h, out))
        return tuple(out)

    @staticmethod
    def _tri(F12, ex, ey, scale_factors, level_sigma2):
        T = Triangulation()
        F12 = np.ascontiguousarray(F12, np.float32).reshape(-1, 9)
        T.n_cams = len(F12)
        sf = np.ascontiguousarray(scale_factors, np.float32); s2 = np.ascontiguousarray(level_sigma2, np.float32)
        T.n_levels = len(sf)
        for c in range(len(F12)):
            for k in range(9):
                T.F12[c][k] = float(F12[c, k])
            T.ex[c] = float(ex[c]); T.ey[c] = float(ey[c])
        T.scale_factors = sf.ctypes.data; T.level_sigma2 = s2.ctypes.data
        return T, (sf, s2)

    def search_for_triangulation(self, a, b, F12, ex, ey, scale_factors, level_sigma2, th_low=50, check_orientation=True):
        T = Triangulation()
        F12 = np.ascontiguousarray(F12, np.float32).reshape(-1, 9)
        T.n_cams = len(F12)
        sf = np.ascontiguousarray(scale_factors, np.float32); s2 = np.ascontiguousarray(level_sigma2, np.float32)
        T.n_levels = len(sf)
        for c in range(len(F12)):
            for k in range(9):
                T.F12[c][k] = float(F12[c, k])
            T.ex[c] = float(ex[c]); T.ey[c] = float(ey[c])
        T.scale_factors = sf.ctypes.data; T.level_sigma2 = s2.ctypes.data
        match = np.full(max(a.n, 1), -1, np.int32); nm = C.c_int()
        ca, cb = a.c(), b.c()
        check(_lib.lib().orbv_search_for_triangulation(self._h, C.byref(ca), C.byref(cb), C.byref(T), th_low, int(check_orientation), ptr(match), C.byref(nm)))
        return nm.value, match[:a.n]


class NewPointsRound:
    """One neighbour of BowSearch.create_new_points_keyframe: what create_new_points_resident takes for `b` (orbv_new_points_round).
    kf1 is the current keyframe's TriKeyframe, the same in every round; cam_enabled is this round's istrian."""

    def __init__(self, b, F12, ex, ey, scale_factors, level_sigma2, kf1, kf2, cam_enabled, ratio_factor, flags_b=None):
        self.b, self.F12, self.ex, self.ey, self.scale_factors, self.level_sigma2 = b, F12, ex, ey, scale_factors, level_sigma2
        self.kf1, self.kf2, self.cam_enabled, self.ratio_factor, self.flags_b = kf1, kf2, cam_enabled, ratio_factor, flags_b


class Keyframe:
    """A Side resident in HBM (orbv_keyframe)."""

    def __init__(self, search, side):
        self._h = C.c_void_p(); self.n = side.n; self._search = search
        cs = side.c()
        check(_lib.lib().orbv_keyframe_create(search._h, C.byref(cs), C.byref(self._h)))

    def set_geometry(self, uright, depth, cos_stereo, xd, yd):
        """The per-feature arrays the triangulation stage reads beyond the search's (orbv_keyframe_set_geometry)."""
        a = [np.ascontiguousarray(v, np.float32) for v in (uright, depth, cos_stereo, xd, yd)]
        assert all(len(v) == self.n for v in a)
        check(_lib.lib().orbv_keyframe_set_geometry(self._search._h, self._h, *[ptr(v) for v in a]))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().orbv_keyframe_destroy(self._h)
            self._h = None

    __del__ = close
