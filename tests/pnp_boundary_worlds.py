"""Boundary worlds of the PnPsolver port (csrc/pnp.hip): problems placed by the model (tests/pnp_model.py) on the port's own decisions,
one float either side -- `error2 < max_err` of pnp_inlier in the hypothesis stage (k_pnp_inliers) and in the refined stage
(k_pnp_refine_inliers), the thresholds of the real form, the non-finite sides, and `c >= min_inliers && c > best` of the record choice
(k_pnp_refine).  Every problem is the dict pnp_worlds.problem() takes and carries its cases
(group, side, stage, hypothesis or record slot, correspondence, expected bit); stage "hyp" reads the hypothesis masks, "ref" the refined
ones.  check_conditions() asserts what the worlds promise on the model and on the host routine.  No tolerance anywhere: bytes.

evaluate() is the model with ONE deliberately wrong rule for the tests of the worlds' teeth; without a rule it is pnp_model's own
statements (pm.errors2, pm.compute_pose, the rule of pm.records) with the poses remembered, and tests/test_pnp_boundary_worlds.py holds
it to pm.ransac_multi."""
import functools
import numpy as np
import pnp_model as pm
import pnp_worlds as pw

f32, f64 = np.float32, np.float64
INF = f32(np.inf)
FLT_MAX = np.finfo(f32).max
SHAPES = ((64, 8), (65, 16), (130, 33), (200, 64))         # (N, H): every bit of a full word, the last bit of a partial one (65 -> 0,
LAST_BITS = {65: 64, 130: 129, 200: 199}                   # 130 -> 1, 200 -> 7); lanes 0, 15, 16 of a k_pnp_hyp workgroup and beyond
RULES = ("inlier_le", "fused_sum", "xc_double", "inv_float", "ue_float", "min_gt", "best_ge")
G_HYP, G_REF, G_REAL, G_NONFINITE = ("hypothesis error2 at its threshold", "refined error2 at its threshold",
                                     "error2 against 5.991 * sigma2 of the octave", "non-finite side")


def bit(words, k, i):
    return bool((int(words[k, i // 64]) >> (i % 64)) & 1)


def up(v):
    return np.nextafter(f32(v), INF)


def camera(w):
    return [float(f32(k)) for k in w["K"]]


# ==================================================================================================== the model, with one wrong rule
def errors2(R, t, K, p3dw, p2d, rule=None):
    """pm.errors2, or -- under a rule -- its statements with that one changed."""
    if rule not in ("fused_sum", "xc_double", "inv_float", "ue_float"):
        return pm.errors2(R, t, K, p3dw, p2d)
    p3dw = np.asarray(p3dw, f32); p2d = np.asarray(p2d, f32)
    X = p3dw.astype(f64)
    fu, fv, uc, vc = [float(k) for k in K]
    with np.errstate(all="ignore"):
        row = lambda r: R[:, None, r, 0] * X[None, :, 0] + R[:, None, r, 1] * X[None, :, 1] + R[:, None, r, 2] * X[None, :, 2] + t[:, None, r]
        Xc, Yc = row(0), row(1)
        if rule != "xc_double":                                    # `Xc` / `Yc` kept in double
            Xc = Xc.astype(f32).astype(f64); Yc = Yc.astype(f32).astype(f64)
        invZc = f32(1) / row(2).astype(f32) if rule == "inv_float" else (1 / row(2)).astype(f32)      # `1.0f / (float)z`
        if rule == "ue_float":                                     # `ue` / `ve` formed in float
            ue = f32(uc) + f32(fu) * Xc.astype(f32) * invZc
            ve = f32(vc) + f32(fv) * Yc.astype(f32) * invZc
            distX = p2d[None, :, 0] - ue; distY = p2d[None, :, 1] - ve
        else:
            ue = uc + fu * Xc * invZc.astype(f64)
            ve = vc + fv * Yc * invZc.astype(f64)
            distX = (p2d[None, :, 0].astype(f64) - ue).astype(f32); distY = (p2d[None, :, 1].astype(f64) - ve).astype(f32)
        if rule == "fused_sum":                                    # fma(distX, distX, distY * distY): the product of two floats is exact in double
            return (distX.astype(f64) * distX.astype(f64) + (distY * distY).astype(f64)).astype(f32)
        return distX * distX + distY * distY


def records(counts, min_inliers, best_start, rule=None):
    out, best = [], best_start
    for h, c in enumerate(counts):
        enough = c > min_inliers if rule == "min_gt" else c >= min_inliers
        better = c >= best if rule == "best_ge" else c > best
        if enough and better:
            best = c
            out.append(h)
    return out


_poses = {}


def _pose(K, P, U):
    """pm.compute_pose of a batch (H, n, 3) / (H, n, 2), remembered: the poses do not depend on the thresholds or on a rule."""
    key = (tuple(K), P.shape, P.tobytes(), U.tobytes())
    if key not in _poses:
        _poses[key] = pm.compute_pose(P, U, np.tile(np.asarray(K, f64), (len(P), 1)))
    return _poses[key]


def evaluate(w, rule=None):
    """What pm.ransac_multi answers for one problem (words, n_inliers, rec, ref_*), with e_hyp (H, N) and e_ref (records, N)."""
    assert rule is None or rule in RULES, rule
    K = camera(w)
    P3 = np.asarray(w["p3dw"], f32); P2 = np.asarray(w["p2d"], f32); thr = np.asarray(w["max_err"], f32)
    q = np.asarray(w["quads"], np.int64).reshape(-1, 4)
    inside = (lambda e: e <= thr[None, :]) if rule == "inlier_le" else (lambda e: e < thr[None, :])
    pose = _pose(K, P3[q].astype(f64), P2[q].astype(f64))
    with np.errstate(all="ignore"):
        e_hyp = errors2(pose["R"], pose["t"], K, P3, P2, rule)
        inl = inside(e_hyp)
    counts = inl.sum(axis=1).astype(np.int32)
    rec = records(counts, w["min_inliers"], w.get("best_start", 0), rule)
    d = {"R": pm.x86_nan(pose["R"]), "t": pm.x86_nan(pose["t"]), "err": pm.x86_nan(pose["err"]), "choice": pose["choice"], "flags": pose["flags"],
         "n_inliers": counts, "words": pm.mask_words(inl), "rec": rec, "e_hyp": e_hyp, "e_ref": np.zeros((len(rec), len(P3)), f32),
         "ref_R": np.zeros((len(rec), 3, 3)), "ref_t": np.zeros((len(rec), 3)), "ref_flags": np.zeros(len(rec), np.int32),
         "ref_n_inliers": np.zeros(len(rec), np.int32), "ref_n_set": np.zeros(len(rec), np.int32),
         "ref_words": np.zeros((len(rec), (len(P3) + 63) // 64), np.uint64)}
    for r, h in enumerate(rec):
        idx = np.nonzero(inl[h])[0]
        rp = _pose(K, P3[idx].astype(f64)[None], P2[idx].astype(f64)[None])
        with np.errstate(all="ignore"):
            d["e_ref"][r] = errors2(rp["R"], rp["t"], K, P3, P2, rule)[0]
            rin = inside(d["e_ref"][r:r + 1])[0]
        d["ref_R"][r] = pm.x86_nan(rp["R"][0]); d["ref_t"][r] = pm.x86_nan(rp["t"][0]); d["ref_flags"][r] = rp["flags"][0]
        d["ref_n_inliers"][r] = rin.sum(); d["ref_n_set"][r] = counts[h]; d["ref_words"][r] = pm.mask_words(rin)
    return d


def _bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64).reshape(-1)


def fields_differing(mod, got):
    """The outputs of the library (hypothesis records, words, refined records, refined words) that differ from a model answer, by name."""
    hyp, words, ref, rwords = got
    out = []
    if len(hyp) != len(mod["n_inliers"]) or words.shape != mod["words"].shape:
        return ["shape"]
    out += [f for f, k in (("R", "R"), ("t", "t"), ("rep_error", "err")) if not np.array_equal(_bits(hyp[f]), _bits(mod[k]))]
    out += [f for f, k in (("choice", "choice"), ("flags", "flags"), ("n_inliers", "n_inliers")) if not np.array_equal(hyp[f], mod[k])]
    out += ["words"] if not np.array_equal(words, mod["words"]) else []
    if list(ref["hyp"]) != list(mod["rec"]):
        return out + ["records %s for %s" % (list(ref["hyp"]), list(mod["rec"]))]
    out += [f for f, k in (("R", "ref_R"), ("t", "ref_t")) if not np.array_equal(_bits(ref[f]), _bits(mod[k]))]
    out += ["refined " + f for f in ("n_set", "n_inliers", "flags") if not np.array_equal(ref[f], mod["ref_" + f])]
    out += ["refined words"] if not np.array_equal(rwords, mod["ref_words"]) else []
    return out


def host(worlds):
    import multi_orb_slam_amd as m
    out = []
    for k in range(0, len(worlds), m.PNP_MAX_BATCH):
        out += m.pnp_ransac_host([pw.problem(m, w) for w in worlds[k:k + m.PNP_MAX_BATCH]])
    return out


# ==================================================================================================== a. hypothesis-stage threshold lanes
HYP_SEEDS = (2101, 2102, 2103, 2104)


def _hyp_lanes():
    """Correspondence i carries its decision under hypothesis h = i mod H: max_err[i] is the model's error2[h, i] (rejected: `e < e`) or
    the next float above (accepted); both parities."""
    out = []
    for (N, H), seed in zip(SHAPES, HYP_SEEDS):
        base = pw.world(N, 0.0, 1.0, seed=seed, H=H, min_inliers=4)
        idx = np.arange(N); h = idx % H
        e = evaluate(base)["e_hyp"][h, idx]
        assert np.isfinite(e).all() and (e > 0).all() and (e < FLT_MAX).all(), (N, H)      # a lane that is not finite or zero is no case
        for parity in (0, 1):
            rejected = idx % 2 == parity
            thr = np.where(rejected, e, np.nextafter(e, INF)).astype(f32)
            cases = [(G_HYP, "rejected" if rejected[i] else "accepted", "hyp", int(h[i]), int(i), bool(~rejected[i])) for i in range(N)]
            out.append(dict(base, max_err=thr, name="hyp_lanes/n%d_h%d/%s rejected" % (N, H, ("even", "odd")[parity]), cases=cases))
    return out


# ==================================================================================================== b. refined-stage threshold lanes
# (N, H, seed, parity of the candidate probes): the shapes in an order that puts every problem behind one of another word count
REF_SPECS = ((64, 8, 2207, 0), (130, 33, 2210, 1), (65, 16, 2207, 0), (200, 64, 2209, 1),
             (64, 8, 2201, 1), (130, 33, 2206, 0), (65, 16, 2204, 1), (200, 64, 2200, 0))


def _ref_lanes():
    """max_err[i] serves both stages, so a probe of the refined stage must stay out of every hypothesis' set: the candidates (every
    second correspondence, noise-free next to set points with 1 px of noise, in no quadruple) start at max_err = 0; a candidate becomes
    a probe of record r where the float above the refined pose's error2 is still at most its error2 under EVERY hypothesis, and gets
    that error2 (rejected) or the float above (accepted).  Every other candidate keeps 0 and is no case.  Both sides of every probe:
    each base is built twice, with the sides exchanged."""
    out = [[], []]
    for N, H, seed, parity in REF_SPECS:
        base = pw.world(N, 0.0, 1.0, seed=seed, H=H, min_inliers=4)
        idx = np.arange(N)
        cand = idx % 2 == parity
        p2d = base["p2d"].copy()
        p2d[cand] = pw.project(base["R"], base["t"], base["p3dw"].astype(f64))[cand].astype(f32)
        others = np.flatnonzero(~cand)
        quads = others[pw.draw_quads(np.random.default_rng(seed + 50), len(others), H)].astype(np.int32)
        max_err = base["max_err"].copy(); max_err[cand] = 0
        w0 = dict(base, p2d=p2d, quads=quads, max_err=max_err)
        ev0 = evaluate(w0)
        rec = ev0["rec"]
        assert 1 <= len(rec) <= pm.MAX_RECORDS, (N, H, rec)
        with np.errstate(all="ignore"):
            floor = np.where(np.isnan(ev0["e_hyp"]), INF, ev0["e_hyp"]).min(axis=0)       # (a NaN error is in no set)
        usable = {}
        for i in np.flatnonzero(cand):
            rs = [r for r in range(len(rec)) if np.isfinite(ev0["e_ref"][r, i]) and ev0["e_ref"][r, i] > 0 and up(ev0["e_ref"][r, i]) <= floor[i]]
            if rs:
                usable[int(i)] = rs[(i // 2) % len(rs)]                                   # spread over the records
        for flip in (0, 1):
            thr = max_err.copy()
            cases = []
            for i, r in usable.items():
                rejected = ((i >> 1) & 1) == flip
                thr[i] = ev0["e_ref"][r, i] if rejected else up(ev0["e_ref"][r, i])
                cases.append((G_REF, "rejected" if rejected else "accepted", "ref", r, i, not rejected))
            w = dict(w0, max_err=thr, cases=cases, n_candidates=int(cand.sum()),
                     name="ref_lanes/n%d_h%d_seed%d/%s" % (N, H, seed, ("first", "second")[flip]))
            # the finished problem: the records and their sets are those of the construction, and no probe entered a set
            ev = evaluate(w)
            assert ev["rec"] == rec and np.array_equal(ev["words"][rec], ev0["words"][rec]) and np.array_equal(ev["n_inliers"], ev0["n_inliers"]), w["name"]
            assert not any(bit(ev["words"], h, i) for i in usable for h in range(H)), w["name"]
            out[flip].append(w)
    return out[0] + out[1]          # (in the order of REF_SPECS twice: every problem stands behind one of another word count)


# ==================================================================================================== c. the thresholds of the real form
REAL_SEED = 2301


def bisect_u(accepted, lo, hi):
    """Adjacent floats (last accepted, first rejected) between lo (accepted) and hi (rejected)."""
    lo, hi = f32(lo), f32(hi)
    assert accepted(lo) and not accepted(hi)
    while up(lo) != hi:
        mid = f32((f64(lo) + f64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = up(lo)
        if accepted(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def _real_thresholds():
    """max_err = sigma2[octave] * 5.991f: correspondence o (octave o, in no quadruple) has its observed u bisected through the host routine
    until its bit under hypothesis o flips; both adjacent problems are kept."""
    import multi_orb_slam_amd as m
    base = pw.world(40, 0.0, 0.0, seed=REAL_SEED, H=8, min_inliers=4)
    base["quads"] = (8 + pw.draw_quads(np.random.default_rng(REAL_SEED + 1), 32, 8)).astype(np.int32)
    assert np.array_equal(base["max_err"][:8], (pw.SIGMA2 * pw.TH2).astype(f32))
    inside, outside = base["p2d"].copy(), base["p2d"].copy()
    for o in range(8):
        def accepted(u, o=o):
            p2d = base["p2d"].copy(); p2d[o, 0] = u
            return bit(m.pnp_ransac_host([pw.problem(m, dict(base, p2d=p2d))])[0][1], o, o)
        inside[o, 0], outside[o, 0] = bisect_u(accepted, base["p2d"][o, 0], base["p2d"][o, 0] + f32(32))
    return [dict(base, p2d=inside, name="real/accepted", cases=[(G_REAL, "accepted, octave %d" % o, "hyp", o, o, True) for o in range(8)]),
            dict(base, p2d=outside, name="real/rejected", cases=[(G_REAL, "rejected, octave %d" % o, "hyp", o, o, False) for o in range(8)])]


# ==================================================================================================== d. non-finite sides
def _non_finite():
    """The depth_zero world with: its depth-zero point twice (thresholds +inf and FLT_MAX), an ordinary point twice, a point observed
    at u = FLT_MAX twice (distX * distX overflows: error2 = +inf), and four coincident points drawn as a third hypothesis, whose pose
    and therefore every error2 is NaN.  Expected: `inf < inf`, `inf < FLT_MAX`, `NaN < inf`, `NaN < FLT_MAX` false; a finite error below
    either threshold true.  The class of every case's error2 is taken from the model and asserted in check_conditions()."""
    w = dict([(x["name"], x) for x in pw.hand_built()])["depth_zero"]
    P, U, E = w["p3dw"], w["p2d"], w["max_err"]
    far = U[10].copy(); far[0] = FLT_MAX
    p3dw = np.concatenate([P, P[11:12], P[10:11], P[10:11], P[10:11], P[10:11], np.repeat(P[9:10], 4, axis=0)]).astype(f32)
    p2d = np.concatenate([U, U[11:12], U[10:11], U[10:11], far[None], far[None], np.repeat(U[9:10], 4, axis=0)]).astype(f32)
    max_err = np.concatenate([E, [FLT_MAX, INF, FLT_MAX, INF, FLT_MAX], np.full(4, pw.TH2, f32)]).astype(f32)
    max_err[11] = INF
    quads = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [17, 18, 19, 20]], np.int32)
    w = dict(w, p3dw=p3dw, p2d=p2d, max_err=max_err, quads=quads, name="non_finite")
    ev = evaluate(w)
    what = {11: "depth zero, +inf", 12: "depth zero, FLT_MAX", 13: "ordinary, +inf", 14: "ordinary, FLT_MAX", 15: "u = FLT_MAX, +inf", 16: "u = FLT_MAX, FLT_MAX"}
    kind = lambda e: "NaN" if np.isnan(e) else "inf" if np.isinf(e) else "finite"
    cases = []
    for i, name in what.items():
        for h in range(3):
            k = kind(ev["e_hyp"][h, i])
            cases.append((G_NONFINITE, "%s < %s" % (k, name.split(", ")[1]), "hyp", h, i, k == "finite"))
        for r in range(len(ev["rec"])):
            k = kind(ev["e_ref"][r, i])
            cases.append((G_NONFINITE, "%s < %s" % (k, name.split(", ")[1]), "ref", r, i, k == "finite"))
    w["cases"] = cases
    w["designed"] = {"hyp": {(h, i): ("NaN" if h == 2 else "inf" if i >= 15 else "finite") for h in range(3) for i in what}}
    return [w]


# ==================================================================================================== e. record choice
RECORD_SEED = 900
G_RECORDS = "record choice"


def _record_choice():
    """`c >= min_inliers && c > best` on its edges: from one world's host counts the first record h0 (count c) and a later record h1
    (count c1 > c); min_inliers at c and c + 1, best_start at c - 1 and c, at c1 - 1 and c1, and the quadruple of h0 repeated as the
    next hypothesis (an equal count, no second record).  Each problem carries the records the design expects."""
    base = pw.world(65, 0.3, 1.0, seed=RECORD_SEED, H=24, min_inliers=4)
    ev = evaluate(base)
    counts, rec = ev["n_inliers"], ev["rec"]
    assert len(rec) >= 2
    h0, h1 = rec[0], rec[1]
    c, c1 = int(counts[h0]), int(counts[h1])
    assert c1 > c >= 4 and h1 > h0
    after = lambda best: pm.records(counts, 4, best)
    rest = [h for h in rec if h != h0]
    out = [dict(base, min_inliers=c, name="records/min_inliers = c", expect=[h for h in rec if counts[h] >= c], side="count == min_inliers"),
           dict(base, min_inliers=c + 1, name="records/min_inliers = c + 1", expect=[h for h in rec if counts[h] >= c + 1], side="count == min_inliers - 1"),
           dict(base, best_start=c - 1, name="records/best_start = c - 1", expect=after(c - 1), side="count == best + 1"),
           dict(base, best_start=c, name="records/best_start = c", expect=after(c), side="count == best"),
           dict(base, best_start=c1 - 1, name="records/best_start = c1 - 1", expect=after(c1 - 1), side="later count == best + 1"),
           dict(base, best_start=c1, name="records/best_start = c1", expect=after(c1), side="later count == best")]
    assert out[0]["expect"][0] == h0 and h0 not in out[1]["expect"] and out[2]["expect"][0] == h0 and h0 not in out[3]["expect"]
    assert out[4]["expect"][0] == h1 and h1 not in out[5]["expect"] and h0 not in out[4]["expect"]
    twice = np.concatenate([base["quads"][:h0 + 1], base["quads"][h0:]])
    out.append(dict(base, quads=twice, name="records/h0 twice", expect=[h0] + [h + 1 for h in rest], side="two consecutive equal counts"))
    # the many-records world: 16 records on the device, the rest from the host routine; then the 17th made ONE inlier better than the 16th
    many = dict(pw.many_records())
    evm = evaluate(many)
    assert len(evm["rec"]) > pm.MAX_RECORDS
    out.append(dict(many, name="records/many_records", expect=list(evm["rec"]), side="more than 16 records"))
    step = _one_inlier_step(many, evm)
    if step is not None:
        out.append(step)
    for w in out:
        w["cases"] = []
    return out


def _one_inlier_step(many, evm):
    """many_records with thresholds of probes that only record 17 (and later hypotheses) accepts set to 0, until record 17 has exactly one
    inlier more than record 16; None if the world does not hold enough such probes."""
    rec, counts = evm["rec"], evm["n_inliers"]
    a, b = rec[pm.MAX_RECORDS - 1], rec[pm.MAX_RECORDS]
    inl = evm["e_hyp"] < np.asarray(many["max_err"], f32)[None, :]
    only = np.flatnonzero(inl[b] & ~inl[:b].any(axis=0))
    drop = int(counts[b] - counts[a] - 1)
    if drop < 0 or len(only) < drop:
        return None
    max_err = np.asarray(many["max_err"], f32).copy()
    max_err[only[:drop]] = 0
    w = dict(many, max_err=max_err, quads=many["quads"][:b + 1], name="records/many_records, 17th = 16th + 1", side="17th record one inlier above the 16th")
    ev = evaluate(w)
    if ev["rec"] != rec[:pm.MAX_RECORDS + 1] or ev["n_inliers"][b] != ev["n_inliers"][a] + 1:
        return None
    w["expect"] = list(ev["rec"])
    return w


# ==================================================================================================== all of them
@functools.lru_cache(maxsize=None)
def problems():
    """Every boundary problem, in the order of the one-batch call."""
    return _hyp_lanes() + _ref_lanes() + _real_thresholds() + _non_finite() + _record_choice()


@functools.lru_cache(maxsize=None)
def host_answers():
    return host(problems())


@functools.lru_cache(maxsize=None)
def model_answers():
    return pm.ransac_multi(problems())


def case_bit(answer, case):
    _, _, stage, k, i, _ = case
    return bit(answer[1] if stage == "hyp" else answer[3], k, i)


def differences(w, got, want):
    """How one answer (the device's) differs from another (the host routine's): fields, then the groups and sides of the cases whose bit
    differs, then the number of differing bits that carry no case."""
    name = w["name"]
    out = []
    for k, f in ((0, "hypothesis records"), (2, "refined records")):
        if got[k].shape != want[k].shape:
            out.append("%s: %d %s for %d" % (name, len(got[k]), f, len(want[k])))
        else:
            out += ["%s: %s, field %s" % (name, f, n) for n in want[k].dtype.names if got[k][n].tobytes() != want[k][n].tobytes()]
    for k, stage in ((1, "hyp"), (3, "ref")):
        if got[k].shape != want[k].shape:
            out.append("%s: %s mask shape %s" % (name, stage, got[k].shape))
            continue
        diff = got[k] ^ want[k]
        mine = [c for c in w["cases"] if c[2] == stage and bit(diff, c[3], c[4])]
        out += ["%s: %s" % (name, x) for x in sorted({"%s[%s]" % (c[0], c[1]) for c in mine})]
        other = sum(bin(int(x)).count("1") for x in diff.reshape(-1)) - len({(c[3], c[4]) for c in mine})
        if other:
            out.append("%s: %d %s bits without a case" % (name, other, stage))
    return out


def wrong_bits(w, answer):
    """The cases whose expected bit is NOT what the answer's mask words hold (the direct assertion, not a comparison of two answers)."""
    return ["%s: expected bit of %s[%s] %s %d, correspondence %d" % ((w["name"],) + c[:5]) for c in w["cases"]
            if c[3] >= (len(answer[1]) if c[2] == "hyp" else len(answer[3])) or case_bit(answer, c) != c[5]]


@functools.lru_cache(maxsize=None)
def check_conditions():
    """-> (the condensed table of groups, sides and counts, {group: cases})"""
    probs, hosts = problems(), host_answers()
    models = [evaluate(w) for w in probs]        # (pm's statements with the poses remembered; tests/test_pnp_boundary_worlds.py holds the
    table = []                                   # host routine to pm.ransac_multi itself)
    counts = {}
    for w, got, mod in zip(probs, hosts, models):
        assert fields_differing(mod, got) == [], (w["name"], fields_differing(mod, got))
        assert wrong_bits(w, got) == [], wrong_bits(w, got)[:5]
        for c in w["cases"]:
            side = c[1].split(",")[0]
            counts.setdefault(c[0], {}).setdefault(side, 0)
            counts[c[0]][side] += 1
    by = lambda prefix: [(k, w) for k, w in enumerate(probs) if w["name"].startswith(prefix)]
    # a. every lane of every word, both parities
    assert sorted({(len(w["p3dw"]), len(w["quads"])) for _, w in by("hyp_lanes")}) == sorted(SHAPES) and len(by("hyp_lanes")) == 8
    for _, w in by("hyp_lanes"):
        N, H = len(w["p3dw"]), len(w["quads"])
        assert len(w["cases"]) == N and [c[4] for c in w["cases"]] == list(range(N)) and all(c[3] == c[4] % H for c in w["cases"])
        assert {0, 15, 16} & {c[3] for c in w["cases"]} == {0, 15, 16} & set(range(H))
    # b. every bit of a full word and the last bit of every partial word carries a refined probe on both sides; a probe on record slot
    #    >= 1 of a problem that stands behind a problem of another word count
    seen = {"rejected": set(), "accepted": set()}
    last = {"rejected": set(), "accepted": set()}
    later_slot = 0
    shares = []
    for k, w in by("ref_lanes"):
        N = len(w["p3dw"])
        ev = evaluate(w)
        for c in w["cases"]:
            assert w["max_err"][c[4]] in (ev["e_ref"][c[3], c[4]], up(ev["e_ref"][c[3], c[4]])) and c[4] not in w["quads"]
            if c[4] < (N // 64) * 64:
                seen[c[1]].add(c[4] % 64)
            if LAST_BITS.get(N) == c[4]:
                last[c[1]].add(N)
        if any(c[3] >= 1 for c in w["cases"]) and len(hosts[k][2]) >= 2:
            assert k >= 1 and (len(probs[k - 1]["p3dw"]) + 63) // 64 != (N + 63) // 64
            later_slot += sum(c[3] >= 1 for c in w["cases"])
        if w["name"].endswith("first"):
            shares.append("%d of %d (%d records)" % (len(w["cases"]), w["n_candidates"], len(ev["rec"])))
    for side in ("rejected", "accepted"):
        assert seen[side] == set(range(64)), (side, sorted(set(range(64)) - seen[side]))
        assert last[side] == set(LAST_BITS), (side, last[side])
    assert later_slot > 0
    # c. eight octaves, both sides, adjacent observations
    (_, wa), (_, wr) = by("real/")
    assert [c[5] for c in wa["cases"]] == [True] * 8 and [c[5] for c in wr["cases"]] == [False] * 8
    assert all(up(wa["p2d"][o, 0]) == wr["p2d"][o, 0] and o not in wa["quads"] for o in range(8))
    assert np.array_equal(np.delete(wa["p2d"].reshape(-1), np.arange(0, 16, 2)), np.delete(wr["p2d"].reshape(-1), np.arange(0, 16, 2)))
    # d. the four false comparisons and the true one, in both stages
    (kd, wd), = by("non_finite")
    evd = evaluate(wd)
    for c in wd["cases"]:
        if c[2] == "hyp":
            assert c[1].split(" < ")[0] == wd["designed"]["hyp"][(c[3], c[4])], c
    sides = {(c[2], c[1]) for c in wd["cases"]}
    assert {("hyp", "%s < %s" % (a, b)) for a in ("finite", "inf", "NaN") for b in ("+inf", "FLT_MAX")} <= sides, sides
    assert len(evd["rec"]) >= 1 and {("ref", "%s < %s" % (a, b)) for a in ("finite", "inf") for b in ("+inf", "FLT_MAX")} <= sides, sides
    # e. the records the design expects, on the model and on the host routine
    names = [w["name"] for _, w in by("records/")]
    assert len(names) >= 8
    for k, w in by("records/"):
        assert models[k]["rec"] == w["expect"] == [int(h) for h in hosts[k][2]["hyp"]], w["name"]
        counts.setdefault(G_RECORDS, {})[w["side"]] = len(w["expect"])
    for g in (G_HYP, G_REF, G_REAL, G_NONFINITE):
        table.append("  %-48s %s" % (g, ", ".join("%s %d" % kv for kv in sorted(counts[g].items()))))
    table.append("  %-48s %s" % (G_RECORDS, "; ".join("%s: %d records" % kv for kv in counts[G_RECORDS].items())))
    table.append("  refined probes usable: %s; %d on a record slot >= 1" % (", ".join(shares), later_slot))
    n_cases = sum(len(w["cases"]) for w in probs)
    table.append("pnp: %d problems, %d cases" % (len(probs), n_cases))
    return "\n".join(table), {g: sum(c.values()) for g, c in counts.items()}
