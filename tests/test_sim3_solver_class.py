"""Sim3Solver (host/Sim3Solver.h) through its driver host/test_sim3: stand-in keyframes and map points built from the worlds of
tests/sim3_worlds.py -- with null entries, bad points, points without an index in their keyframe and features of the second camera --
the triples the class drew fed to the model, and every iterate(5, ...) / find and the three getters compared with the model's
`iterate`.  Below SIM3_HOST_BELOW (hypotheses x correspondences) a preparation takes the library's host routine (no device needed);
from there on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sim3_model as sm
import sim3_worlds as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_sim3")
F = np.float32
SIM3_HOST_BELOW = 4096


def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def rigid(seed):
    rng = np.random.RandomState(seed)
    T = np.eye(4)
    T[:3, :3] = sw.rot(rng.randn(3), rng.uniform(0.2, 2.0))
    T[:3, 3] = rng.uniform(-3, 3, 3)
    return T.astype(F)


class Case:
    """A solver's inputs as the reference's objects hold them, made from a world's camera-frame points."""

    def __init__(self, W, seed, min_inliers=15, max_its=300, protocol=0):
        rng = np.random.RandomState(seed)
        n = len(W["x3dc1"])
        self.W, self.min_inliers, self.max_its, self.protocol = W, min_inliers, max_its, protocol
        self.T1, self.T2 = rigid(seed + 1), rigid(seed + 2)
        back = lambda T, X: ((X.astype(np.float64) - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)).astype(F)
        Xw1, Xw2 = back(self.T1, W["x3dc1"]), back(self.T2, W["x3dc2"])
        self.sigma2 = np.array(sw.level_sigma2(), F)
        # keyframe 1: the correspondences at every feature but each fourth one (those get the special entries); keyframe 2: shuffled
        self.mN1 = n + n // 3 + 6
        slots = [i for i in range(self.mN1) if i % 4 != 3][:n]
        specials = [i for i in range(self.mN1) if i not in set(slots)]
        self.n2 = n + 5
        idx2 = rng.permutation(self.n2)[:n]
        self.oct1 = rng.randint(0, sw.N_LEVELS, self.mN1); self.cam1 = np.zeros(self.mN1, np.int64)
        self.oct2 = rng.randint(0, sw.N_LEVELS, self.n2); self.cam2 = np.zeros(self.n2, np.int64)
        # entry: (has1, bad1, idx1, X1w, has2, bad2, idx2, X2w)
        zero = np.zeros(3, F)
        self.entries = [(0, 0, -1, zero, 0, 0, -1, zero)] * self.mN1
        for k, i1 in enumerate(slots):
            self.oct1[i1], self.cam1[i1] = W["octave"][0][k], W["cam1"][k]
            self.oct2[idx2[k]], self.cam2[idx2[k]] = W["octave"][1][k], W["cam2"][k]
            self.entries[i1] = (1, 0, i1, Xw1[k], 1, 0, int(idx2[k]), Xw2[k])
        kinds = ["no_match", "no_point1", "bad1", "bad2", "no_index1", "no_index2", "good_elsewhere"]
        for j, i1 in enumerate(specials):
            kind = kinds[j % len(kinds)]
            p1, p2 = rng.uniform(-2, 2, 3).astype(F), rng.uniform(-2, 2, 3).astype(F)
            i2 = int(rng.randint(0, self.n2))
            self.entries[i1] = {"no_match": (1, 0, i1, p1, 0, 0, -1, zero), "no_point1": (0, 0, -1, zero, 1, 0, i2, p2),
                                "bad1": (1, 1, i1, p1, 1, 0, i2, p2), "bad2": (1, 0, i1, p1, 1, 1, i2, p2),
                                "no_index1": (1, 0, -1, p1, 1, 0, i2, p2), "no_index2": (1, 0, i1, p1, 1, 0, -1, p2),
                                # a point whose index in keyframe 1 is ANOTHER feature: octave and camera come from that one
                                "good_elsewhere": (1, 0, slots[j % len(slots)], p1, 1, 0, i2, p2)}[kind]

    def lines(self):
        W = self.W
        out = ["1", "%d %d %d %d" % (int(W["fix_scale"]), self.min_inliers, self.max_its, self.protocol), hexf(W["calib"])]
        for T, K, octs, cams in ((self.T1, W["K1"], self.oct1, self.cam1), (self.T2, W["K2"], self.oct2, self.cam2)):
            out += [hexf(T), hexf(K), "%d" % len(self.sigma2), hexf(self.sigma2), "%d" % len(octs)]
            out += ["%d %d" % (o, c) for o, c in zip(octs, cams)]
        out.append("%d" % self.mN1)
        for h1, b1, i1, X1, h2, b2, i2, X2 in self.entries:
            out.append("%d %d %d %s %d %d %d %s" % (h1, b1, i1, hexf(X1), h2, b2, i2, hexf(X2)))
        return out

    def filtered(self):
        """The constructor's loop (src/Sim3Solver.cc:76-141) -> the model's world."""
        def cam_frame(T, X):
            T = T.astype(F)
            return np.stack([sm.cv_gemm3(T[r, 0], T[r, 1], T[r, 2], X[:, 0], X[:, 1], X[:, 2], 1.0, T[r, 3], 1.0) for r in range(3)], axis=1)
        rows = [(i, e) for i, e in enumerate(self.entries) if e[4] and e[0] and not e[1] and not e[5] and e[2] >= 0 and e[6] >= 0]
        idx1 = np.array([e[2] for _, e in rows], np.int64); idx2 = np.array([e[6] for _, e in rows], np.int64)
        X1 = np.array([e[3] for _, e in rows], F).reshape(-1, 3); X2 = np.array([e[7] for _, e in rows], F).reshape(-1, 3)
        err = lambda octs: np.array([F(int(9.210 * float(self.sigma2[o]))) for o in octs], F)
        W = self.W
        return dict(K1=W["K1"], K2=W["K2"], Rcam21=W["Rcam21"], tcam21=W["tcam21"], fix_scale=W["fix_scale"], x3dc1=cam_frame(self.T1, X1),
                    x3dc2=cam_frame(self.T2, X2), cam1=self.cam1[idx1], cam2=self.cam2[idx2], max_err1=err(self.oct1[idx1]),
                    max_err2=err(self.oct2[idx2])), np.array([i for i, _ in rows], np.int64)


def run_driver(tmp_path, cases, seed, mode):
    lines = ["%d %d %d" % (len(cases), seed, mode)]
    for c in cases:
        lines += ["0"] if c is None else c.lines()
    f = tmp_path / "solvers.txt"
    f.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["timeout", "-k", "10", "120", DRIVER, str(f)], capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = [], None
    for line in p.stdout.splitlines():
        t = line.split()
        if t[0] == "null":
            out.append(None)
        elif t[0] == "triples":
            cur = dict(triples=np.array(t[2:], np.int32).reshape(-1, 3), calls=[], best=None)
            assert len(cur["triples"]) == int(t[1])
            out.append(cur)
        elif t[0] == "call":
            if t[1] == "-":
                T, rest = None, t[2:]
            else:
                T, rest = np.array([int(x, 16) for x in t[1:17]], np.uint32).view(np.float32), t[17:]
            cur["calls"].append((T, int(rest[0]), int(rest[1]), np.array([ch == "1" for ch in rest[2]]) if rest[2] != "-" else np.zeros(0, bool)))
        elif t[0] == "best":
            cur["best"] = None if t[1] == "-" else np.array([int(x, 16) for x in t[1:]], np.uint32).view(np.float32)
    assert len(out) == len(cases)
    return out


def check_against_model(case, got):
    Wm, indices1 = case.filtered()
    N = len(indices1)
    H = sm.iterations(0.99, case.min_inliers, case.max_its, N)
    triples = got["triples"]
    if N < case.min_inliers:
        assert len(triples) == 0
    else:
        assert len(triples) == H                                   # every iteration of mRansacMaxIts was drawn up front
        assert triples.min() >= 0 and triples.max() < N
        assert (triples[:, 0] != triples[:, 1]).all() and (triples[:, 0] != triples[:, 2]).all() and (triples[:, 1] != triples[:, 2]).all()
    Wm["triples"] = triples
    rec, masks, _, _ = sm.evaluate(Wm, "device")                   # (what the library computes, bit for bit)
    it = sm.Iterate(rec["n_inliers"], N, case.min_inliers, H)
    calls = 0
    for T, no_more, n_inliers, vb in got["calls"]:
        h, want_no_more, want_n = it.iterate(H if case.protocol == 1 else 5)
        if case.protocol == 1:
            want_no_more = True                                    # (find has no bNoMore: the driver prints 1)
        assert (no_more == 1) == want_no_more and n_inliers == want_n, (calls, h)
        want_vb = np.zeros(case.mN1, bool)
        if h < 0:
            assert T is None
        else:
            assert T is not None and T.tobytes() == rec["T12"][h].tobytes(), (calls, h)
            bit = (masks[h][np.arange(N) >> 6] >> (np.arange(N) & 63).astype(np.uint64)) & np.uint64(1)
            want_vb[indices1[bit.astype(bool)]] = True
        assert np.array_equal(vb, want_vb), (calls, h)
        calls += 1
    if case.protocol == 0:
        assert got["calls"][-1][1] == 1                            # the driver went on until bNoMore
    if it.best < 0:
        assert got["best"] is None
    else:
        want = np.concatenate([rec["R12"][it.best], rec["t12"][it.best], rec["s12"][it.best:it.best + 1]])
        assert got["best"].tobytes() == want.tobytes()
    return rec, it


def libc_randi(seed):
    """DUtils::Random::RandomInt(0, n - 1) on the C library's own rand() after srand(seed)."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    libc.rand.restype = ctypes.c_int
    return lambda n: int((float(libc.rand()) / (2147483647.0 + 1.0)) * n)


def small(seed, n, **kw):
    return sw.generate(seed, n, **kw)


CPU_CASES = {
    "n12_below_min": dict(W=dict(n=12), min_inliers=15),
    "n15_equal_min": dict(W=dict(n=15), min_inliers=None),        # (None: exactly the number of correspondences the constructor keeps)
    "n20_wrong30_two_cams": dict(W=dict(n=20, wrong=0.3, noise=1.0, cams=(0.3, 0.3)), min_inliers=15),
    "n30_fixed_scale": dict(W=dict(n=30, fix_scale=True, wrong=0.3, noise=1.0), min_inliers=15),
    "n36_free_0.7_find": dict(W=dict(n=36, s=0.7, wrong=0.3, noise=1.0, cams=(0.0, 0.4)), min_inliers=15, protocol=1),
    "n36_all_wrong": dict(W=dict(n=36, wrong=1.0, noise=1.0), min_inliers=15),
    "n25_min6": dict(W=dict(n=25, s=1.4, wrong=0.3, noise=1.0), min_inliers=6, max_its=40),
}


def make_case(name, spec, seed=300):
    seed += sum(map(ord, name))
    case = Case(small(seed, **spec["W"]), seed, min_inliers=spec["min_inliers"] or 0, max_its=spec.get("max_its", 300), protocol=spec.get("protocol", 0))
    if spec["min_inliers"] is None:
        case.min_inliers = len(case.filtered()[1])
    return case


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_class_below_the_threshold_takes_the_host_routine(tmp_path, name):
    case = make_case(name, CPU_CASES[name])
    Wm, indices1 = case.filtered()
    H = sm.iterations(0.99, case.min_inliers, case.max_its, len(indices1))
    assert H * len(indices1) < SIM3_HOST_BELOW
    (got,) = run_driver(tmp_path, [case], seed=17, mode=0)
    rec, it = check_against_model(case, got)
    # the drawing itself: the take-and-swap procedure on RandomInt's arithmetic over the C library's rand()
    if len(indices1) >= case.min_inliers:
        assert got["triples"].tolist() == sm.draw_triples(len(indices1), H, libc_randi(17)).tolist()
    if name == "n12_below_min":
        assert len(got["calls"]) == 1 and got["calls"][0][0] is None and got["best"] is None
    if name == "n15_equal_min":
        assert H == 1 and len(got["calls"]) == 1 and got["calls"][0][0] is None and got["best"] is not None   # N > N is false: the best is kept, nothing returned
    if name == "n30_fixed_scale":
        assert any(c[0] is not None for c in got["calls"]) and rec["s12"][it.best] == 1.0
    if name == "n36_all_wrong":
        assert all(c[0] is None for c in got["calls"])


def test_the_special_entries_are_filtered_as_the_constructor_does(tmp_path):
    case = make_case("n20_wrong30_two_cams", CPU_CASES["n20_wrong30_two_cams"])
    Wm, indices1 = case.filtered()
    # every slot survives, and of the special entries only the points that are good but indexed elsewhere
    elsewhere = [i for i, e in enumerate(case.entries) if e[0] and e[4] and not e[1] and not e[5] and e[2] >= 0 and e[6] >= 0 and e[2] != i]
    assert len(indices1) == 20 + len(elsewhere) and len(elsewhere) >= 1
    assert Wm["cam1"].any() and Wm["cam2"].any()


def test_class_under_asan_ubsan(tmp_path, monkeypatch):
    """The sanitized build of the class and its driver (host/Makefile `san`) on the cases that need no device: a report fails the run."""
    host = os.path.dirname(DRIVER)
    subprocess.check_call(["make", "-s", "-C", host, "test_sim3_san"], timeout=900)
    monkeypatch.setattr("test_sim3_solver_class.DRIVER", os.path.join(host, "test_sim3_san"))
    monkeypatch.setenv("ASAN_OPTIONS", "detect_leaks=1:abort_on_error=0:exitcode=99")
    monkeypatch.setenv("UBSAN_OPTIONS", "print_stacktrace=1:halt_on_error=1:exitcode=98")
    cases = [make_case(n, CPU_CASES[n]) for n in ("n12_below_min", "n20_wrong30_two_cams", "n36_free_0.7_find")]
    for case, got in zip(cases, run_driver(tmp_path, cases, seed=5, mode=0)):
        check_against_model(case, got)


GPU_SPECS = [dict(n=64, wrong=0.3, noise=1.0, cams=(0.2, 0.2)), dict(n=300, s=0.7, wrong=0.6, noise=1.0), dict(n=2000, fix_scale=True, wrong=0.3, noise=1.0, cams=(0.3, 0.0)),
             dict(n=100, s=1.4, wrong=0.3, noise=1.0, rig="wide", cams=(0.4, 0.4)), dict(n=12), dict(n=500, wrong=0.3, noise=0.0),
             dict(n=1000, s=0.7, wrong=0.6, noise=1.0, cams=(0.0, 0.3)), dict(n=40, wrong=0.3, noise=1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_solvers", [1, 3, 8])
def test_prepare_evaluates_every_solver_in_one_call_on_the_device(tmp_path, n_solvers):
    import torch  # noqa: F401
    cases = [Case(small(500 + i, **GPU_SPECS[i]), 500 + i, protocol=1 if i == 2 else 0) for i in range(n_solvers)]
    if n_solvers > 1:
        cases[1] = None                                            # a discarded candidate: vpSim3Solvers[i] stays null
    got = run_driver(tmp_path, cases, seed=23, mode=1)
    # Prepare draws for every solver before anything else happens in the process: ONE stream of the C library's rand(), solver after solver
    randi = libc_randi(23)
    for c, g in zip(cases, got):
        if c is None:
            assert g is None
            continue
        check_against_model(c, g)
        N = len(c.filtered()[1])
        if N >= c.min_inliers:
            assert g["triples"].tolist() == sm.draw_triples(N, len(g["triples"]), randi).tolist()
    # Each solver preparing itself on its first iterate: every one equals the model on ITS OWN triples.  rand() is one process-wide
    # stream, and a solver's device call lies between its draws and the next solver's: the device runtime draws from the same stream
    # when it is first used, so only the first solver's triples are those of the run above (the deviation INTEGRATION.md describes:
    # the class does not own the stream's position).
    single = run_driver(tmp_path, cases, seed=23, mode=0)
    first = True
    for c, g, s in zip(cases, got, single):
        if c is None:
            assert s is None
            continue
        check_against_model(c, s)
        if first:
            assert g["triples"].tolist() == s["triples"].tolist() and len(g["calls"]) == len(s["calls"])
            for a, b in zip(g["calls"], s["calls"]):
                assert (a[0] is None) == (b[0] is None) and (a[0] is None or a[0].tobytes() == b[0].tobytes()) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3])
            first = False
