"""Second, independent restatement of the BoW-gated searches (ORBmatcher.cc:206-388, :996-1165, :1364-1786) in NumPy over
dict-of-lists feature vectors: what tests/test_oracle_bow.py holds the oracle (oracle/bow_oracle.cpp) against on random worlds and
tests/test_bow_boundary_worlds.py on the boundary worlds of tests/bow_boundary_worlds.py.  No GPU, no product code.

Both searches take `rules`, names of deliberately WRONG rules (RULES_BOW / RULES_TRI; the default () is the reference's behaviour), and a
`trace`: a dict that receives, per query (feature index of side a), the distances, the value pair of every comparison, the histogram
bin and the gate that turned each close-enough candidate away.  The distances of a query to its node are one vectorised expression:
the boundary worlds have nodes of 1 600 candidates."""
import math
import numpy as np

f32 = np.float32
HISTO_LENGTH = 30
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)

RULES_COMMON = ("bin_half_even",        # rotation bin rounded half-to-even (rintf / lrintf) instead of half-away (round)
                "bin_divide",           # rot / 30 instead of rot * (1.0f / 30)
                "maxima_double")        # (float)m2 < 0.1f * (float)m1 evaluated in double
RULES_BOW = RULES_COMMON + (
    "th_swapped",                       # mode 0 `<`, mode 1 `<=` on the distance threshold
    "ratio_double",                     # (float)best < nnratio * (float)second with the product in double
    "claims_ignored",                   # an accepted match hides nothing
    "claims_after_rotation",            # mode 0: only the matches that survive the rotation filter hide their feature
    "mode1_ignores_b_flag",             # mode 1 looks at candidates of b without a usable MapPoint
    "mode0_honours_b_flag",             # mode 0 skips them
    "last_on_ties")                     # `<=` in the best-distance update: the last of equal candidates wins
RULES_TRI = RULES_COMMON + (
    "epipole_le",                       # dex^2 + dey^2 <= 100 * scale rejects
    "epipole_always",                   # the epipole gate whatever the stereo flags
    "dsqr_float",                       # dsqr < 3.84f * sigma2 in float
    "dsqr_le",                          # dsqr <= 3.84 * sigma2
    "num_fma",                          # a * x2 + b * y2 contracted into a multiply-add: one rounding less in the numerator
    "th_ge_rejects",                    # dist >= th_low is turned away
    "den_zero_accepted",                # den == 0 passes
    "camera_ignored",                   # candidates of another camera count
    "shadow",                           # the nearest candidate is chosen before the gates: one that fails them hides a farther one that passes
    "first_on_ties")                    # `dist >= bestDist` is skipped: the first of equal candidates wins


def popcount(a, b):
    return int(_POP8[np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)].sum())


def distances(d1, descs):
    """Hamming distances of one descriptor to the rows of `descs`."""
    return _POP8[np.asarray(descs, np.uint8).reshape(-1, 32) ^ np.asarray(d1, np.uint8)].sum(axis=1)


def py_three_maxima(sizes, rules=(), trace=None):
    m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1: m3, i3, m2, i2, m1, i1 = m2, i2, m1, i1, s, i
        elif s > m2: m3, i3, m2, i2 = m2, i2, s, i
        elif s > m3: m3, i3 = s, i
    if "maxima_double" in rules:
        lim = np.float64(f32(0.1)) * np.float64(m1)
    else:
        lim = f32(0.1) * f32(m1)
    if trace is not None:
        trace["maxima"] = (m1, m2, m3, float(lim))
    if f32(m2) < lim: i2 = i3 = -1      # (a float32 against a float64 compares in double)
    elif f32(m3) < lim: i3 = -1
    return i1, i2, i3


def py_rot(a1, a2):
    rot = f32(f32(a1) - f32(a2))
    if rot < 0: rot = f32(rot + f32(360.0))
    return rot


def py_bin(a1, a2, rules=()):
    rot = py_rot(a1, a2)
    v = float(f32(rot / f32(30.0))) if "bin_divide" in rules else float(f32(rot * f32(1.0 / 30)))
    if "bin_half_even" in rules:
        b = int(np.rint(v))
    else:
        b = int(math.floor(v + 0.5))   # round half away from zero, v >= 0
    return 0 if b == 30 else b


def fv_dict(s):
    return {int(k): s["items"][s["node_start"][i]:s["node_start"][i + 1]].tolist() for i, k in enumerate(s["node_id"])}


def _filter(match, hist, rules, trace):
    """The rotation filter: every match outside the three maxima goes.  -> number removed"""
    keep = py_three_maxima([len(h) for h in hist], rules, trace)
    gone = 0
    for i, h in enumerate(hist):
        if i in keep: continue
        for j in h: match[j] = -1; gone += 1
    return gone


def py_search_by_bow(a, b, mode, th_low, nnratio, check_ori, rules=(), trace=None, _silent=()):
    """-> (nmatches, match).  trace[idx1] = dict(best, second, bi, th=(best, th_low), ratio=(float best, product), accepted, bin, rot)."""
    assert all(r in RULES_BOW for r in rules), rules
    if "claims_after_rotation" in rules and mode == 0 and check_ori and not _silent:
        # the matches the filter removes never hid anything: found with the right rule first, then replayed without their claims
        t0 = {}
        _, m0 = py_search_by_bow(a, b, mode, th_low, nnratio, False, (), t0)
        _, m1 = py_search_by_bow(a, b, mode, th_low, nnratio, True, ())
        removed = {int(m0[i]) for i in range(len(m0)) if m0[i] >= 0 and m1[i] < 0}
        return py_search_by_bow(a, b, mode, th_low, nnratio, check_ori, rules, trace, _silent=removed or {-1})
    fa, fb = fv_dict(a), fv_dict(b)
    adesc, bdesc = np.asarray(a["desc"], np.uint8).reshape(-1, 32), np.asarray(b["desc"], np.uint8).reshape(-1, 32)
    bflags = np.asarray(b["flags"])
    n_out = len(bdesc) if mode == 0 else len(adesc)
    match = [-1] * n_out
    hidden = np.zeros(len(bdesc), bool)           # mode 0: vpMapPointMatches[idx2] set; mode 1: vbMatched2[idx2]
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    b_flag = (mode == 1 and "mode1_ignores_b_flag" not in rules) or (mode == 0 and "mode0_honours_b_flag" in rules)
    strict = (mode == 1) != ("th_swapped" in rules)
    for node in sorted(set(fa) & set(fb)):
        cand = np.asarray(fb[node], np.int64)
        for i1 in fa[node]:
            if not a["flags"][i1] & 1: continue
            ok = ~hidden[cand] if "claims_ignored" not in rules else np.ones(len(cand), bool)
            if b_flag: ok &= (bflags[cand] & 1) != 0
            live = cand[ok]
            d = distances(adesc[i1], bdesc[live]) if len(live) else np.zeros(0, np.int64)
            b1, b2, bi = 256, 256, -1
            if len(d):
                order = np.sort(d)
                if order[0] < 256:
                    b1 = int(order[0])
                    at = np.flatnonzero(d == b1)
                    bi = int(live[at[-1] if "last_on_ties" in rules else at[0]])
                    if "last_on_ties" in rules:   # `<=`: every equal candidate pushes the one before it into second place
                        b2 = b1 if len(at) > 1 else (int(order[1]) if len(order) > 1 else 256)
                    else:
                        b2 = int(order[1]) if len(order) > 1 else 256
            under = b1 < th_low if strict else b1 <= th_low
            if "ratio_double" in rules:
                prod = np.float64(f32(nnratio)) * np.float64(b2)    # (a float32 against a float64 compares in double)
            else:
                prod = f32(f32(nnratio) * f32(b2))
            accepted = bool(under and f32(b1) < prod)
            tr = dict(best=b1, second=b2, bi=bi, th=(b1, th_low), ratio=(float(b1), float(prod)), accepted=accepted, bin=-1)
            if accepted:
                if mode == 0:
                    match[bi] = i1
                else:
                    match[i1] = bi
                if i1 not in _silent:
                    hidden[bi] = True
                if check_ori:
                    tr["rot"] = py_rot(a["angle"][i1], b["angle"][bi])
                    tr["bin"] = py_bin(a["angle"][i1], b["angle"][bi], rules)
                    hist[tr["bin"]].append(bi if mode == 0 else i1)
                nm += 1
            if trace is not None:
                trace[int(i1)] = tr
    if check_ori:
        nm -= _filter(match, hist, rules, trace)
    if mode == 0:
        nm = sum(1 for v in match if v >= 0)      # (an overwritten word counted twice on the way: claims_ignored only)
    return nm, match


def epipolar_line(F, x1, y1):
    x1, y1 = f32(x1), f32(y1)
    la = f32(f32(f32(x1 * F[0]) + f32(y1 * F[3])) + F[6]); lb = f32(f32(f32(x1 * F[1]) + f32(y1 * F[4])) + F[7])
    lc = f32(f32(f32(x1 * F[2]) + f32(y1 * F[5])) + F[8])
    return la, lb, lc


def epipolar_dsqr(la, lb, lc, x2, y2, rules=()):
    """-> (dsqr, den) of CheckDistEpipolarLine in float (:167-184); dsqr is None when den == 0."""
    x2, y2 = f32(x2), f32(y2)
    if "num_fma" in rules:
        num = f32(f32(float(la) * float(x2) + float(f32(lb * y2))) + lc)
    else:
        num = f32(f32(f32(la * x2) + f32(lb * y2)) + lc)
    den = f32(f32(la * la) + f32(lb * lb))
    if den == 0:
        return None, den
    return f32(f32(num * num) / den), den


def dsqr_passes(dsqr, sigma2, rules=()):
    """dsqr < 3.84 * sigma2[octave]: the float widened, the product in double."""
    if "dsqr_float" in rules:
        lim = f32(f32(3.84) * f32(sigma2))
        return bool(dsqr <= lim) if "dsqr_le" in rules else bool(dsqr < lim)
    lim = 3.84 * float(sigma2)
    return float(dsqr) <= lim if "dsqr_le" in rules else float(dsqr) < lim


def epipole_rejects(ex, ey, x2, y2, scale, rules=()):
    """-> (rejects, lhs, rhs): dex^2 + dey^2 < 100 * scale[octave], all float."""
    dx, dy = f32(f32(ex) - f32(x2)), f32(f32(ey) - f32(y2))
    lhs = f32(f32(dx * dx) + f32(dy * dy)); rhs = f32(f32(100) * f32(scale))
    return (bool(lhs <= rhs) if "epipole_le" in rules else bool(lhs < rhs)), lhs, rhs


def py_triangulation(a, b, F12, ex, ey, sf, s2, th_low, check_ori, rules=(), trace=None):
    """-> (nmatches, match).  trace[idx1] = dict(best, bi, gates = {idx2: (gate, lhs, rhs)} of every usable candidate of the camera within
    th_low, bin, rot); gate is one of "pass", "epipole", "den", "dsqr"."""
    assert all(r in RULES_TRI for r in rules), rules
    fa, fb = fv_dict(a), fv_dict(b)
    adesc, bdesc = np.asarray(a["desc"], np.uint8).reshape(-1, 32), np.asarray(b["desc"], np.uint8).reshape(-1, 32)
    bflags, bcam = np.asarray(b["flags"]), np.asarray(b["cam_of"])
    match = [-1] * len(adesc); hist = [[] for _ in range(HISTO_LENGTH)]; nm = 0
    for node in sorted(set(fa) & set(fb)):
        cand = np.asarray(fb[node], np.int64)
        for i1 in fa[node]:
            if not a["flags"][i1] & 1: continue
            cam = int(a["cam_of"][i1]); st1 = bool(a["flags"][i1] & 2)
            ok = (bflags[cand] & 1) != 0
            if "camera_ignored" not in rules: ok &= bcam[cand] == cam
            live = cand[ok]
            d = distances(adesc[i1], bdesc[live]) if len(live) else np.zeros(0, np.int64)
            near = d < th_low if "th_ge_rejects" in rules else d <= th_low
            la, lb, lc = epipolar_line(F12[cam], a["x"][i1], a["y"][i1])
            gates = {}
            for i2, di in zip(live[near].tolist(), d[near].tolist()):      # (a handful: only these reach the gates)
                x2, y2, o2 = b["x"][i2], b["y"][i2], int(b["octave"][i2])
                gate = ("pass", 0.0, 0.0)
                if "epipole_always" in rules or (not st1 and not b["flags"][i2] & 2):
                    rej, lhs, rhs = epipole_rejects(ex[cam], ey[cam], x2, y2, sf[o2], rules)
                    if rej: gate = ("epipole", float(lhs), float(rhs))
                if gate[0] == "pass":
                    dsqr, den = epipolar_dsqr(la, lb, lc, x2, y2, rules)
                    if dsqr is None:
                        if "den_zero_accepted" not in rules: gate = ("den", 0.0, 0.0)
                    elif not dsqr_passes(dsqr, s2[o2], rules): gate = ("dsqr", float(dsqr), 3.84 * float(s2[o2]))
                    else: gate = ("pass", float(dsqr), 3.84 * float(s2[o2]))
                gates[int(i2)] = (gate, int(di))
            best, bi = th_low, -1
            pool = [(i2, di, g[0] == "pass") for i2, (g, di) in gates.items()]
            if "shadow" in rules:
                if pool:
                    dmin = min(di for _, di, _ in pool)
                    i2, di, passes = [p for p in pool if p[1] == dmin][-1]
                    if passes: best, bi = di, i2
            else:
                passing = [p for p in pool if p[2]]
                if passing:
                    dmin = min(di for _, di, _ in passing)
                    tied = [p for p in passing if p[1] == dmin]
                    i2, di, _ = tied[0] if "first_on_ties" in rules else tied[-1]   # `dist > bestDist` skips: an equal, later one replaces
                    best, bi = di, i2
            tr = dict(best=best, bi=bi, gates={k: v[0] for k, v in gates.items()}, bin=-1)
            if bi >= 0:
                match[i1] = bi; nm += 1
                if check_ori:
                    tr["rot"] = py_rot(a["angle"][i1], b["angle"][bi])
                    tr["bin"] = py_bin(a["angle"][i1], b["angle"][bi], rules)
                    hist[tr["bin"]].append(i1)
            if trace is not None:
                trace[int(i1)] = tr
    if check_ori:
        nm -= _filter(match, hist, rules, trace)
    return nm, match
