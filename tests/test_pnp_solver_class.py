"""PnPsolver (host/PnPsolver.h) through its driver host/test_pnp: stand-in frames and map points built from the worlds of
tests/pnp_worlds.py -- with null entries and bad points -- the quadruples the class drew fed to the model, and every iterate(5, ...)
until bNoMore, the calls after it (they run past mRansacMaxIts: continuation blocks with best_start, the best record carried along) and
find compared with the model's `iterate`.  Below PNP_HOST_BELOW (hypotheses x correspondences) an evaluation takes the library's host
routine (no device needed); from there on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pnp_model as pm
import pnp_worlds as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_pnp")
F = np.float32
PARAMS = dict(probability=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5)   # Tracking::Relocalization's


def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


class Case:
    """A solver's inputs as the reference's objects hold them: the world's correspondences at every feature but each fourth one, which
    is a null entry, a bad point or a feature without a match."""

    def __init__(self, W, seed, protocol=0, extra=0):
        rng = np.random.RandomState(seed)
        n = len(W["p3dw"])
        self.W, self.protocol, self.extra = W, protocol, extra
        self.nf = n + n // 3 + 5
        slots = [i for i in range(self.nf) if i % 4 != 3][:n]
        self.octave = rng.randint(0, pw.LEVELS, self.nf)
        self.xy = rng.uniform(0, 480, (self.nf, 2)).astype(F)
        self.entries = [(0, 0, np.zeros(3, F))] * self.nf
        for k, i in enumerate(slots):
            self.octave[i] = k % pw.LEVELS
            self.xy[i] = W["p2d"][k]
            self.entries[i] = (1, 0, W["p3dw"][k])
        for j, i in enumerate(i for i in range(self.nf) if i not in set(slots)):
            self.entries[i] = [(0, 0, np.zeros(3, F)), (1, 1, rng.uniform(-2, 2, 3).astype(F)), (0, 1, rng.uniform(-2, 2, 3).astype(F))][j % 3]
        self.kept = np.array([i for i, e in enumerate(self.entries) if e[0] and not e[1]], np.int64)
        assert list(self.kept) == slots

    def lines(self):
        out = ["1", "%d %d" % (self.protocol, self.extra), hexf(self.W["K"]), "%d" % pw.LEVELS, hexf(pw.SIGMA2), "%d" % self.nf]
        out += ["%d %s" % (o, hexf(p)) for o, p in zip(self.octave, self.xy)]
        out += ["%d %d %s" % (h, b, hexf(X)) for h, b, X in self.entries]
        return out


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
        if t[0] == "host_below":
            run_driver.host_below = int(t[1])                      # PNP_HOST_BELOW as the driver was built with it
        elif t[0] == "null":
            out.append(None)
        elif t[0] == "quads":
            cur = dict(quads=np.array(t[2:], np.int32).reshape(-1, 4), calls=[])
            assert len(cur["quads"]) == int(t[1])
            out.append(cur)
        elif t[0] == "call":
            if t[1] == "-":
                T, rest = None, t[2:]
            else:
                T, rest = np.array([int(x, 16) for x in t[1:17]], np.uint32).view(np.float32), t[17:]
            cur["calls"].append((T, int(rest[0]), int(rest[1]), np.array([ch == "1" for ch in rest[2]]) if rest[2] != "-" else np.zeros(0, bool)))
    assert len(out) == len(cases)
    return out


def pose16(R, t):
    T = np.eye(4, dtype=F)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3).astype(F); T[:3, 3] = np.asarray(t, np.float64).astype(F)
    return T.reshape(16)


def check_against_model(case, got):
    """Every call of the driver against PnPsolver::iterate transcribed (pnp_model.IterateModel) on the quadruples the class drew."""
    W = case.W
    N = len(case.kept)
    max_its, min_inl, _ = pm.parameters(N, **PARAMS)
    quads = got["quads"]
    if N < min_inl:
        assert len(quads) == 0 and len(got["calls"]) == 1 + case.extra
        for T, no_more, n_inliers, vb in got["calls"]:
            assert T is None and no_more == 1 and n_inliers == 0 and len(vb) == 0
        return None
    assert len(quads) >= max_its and quads.min() >= 0 and quads.max() < N
    assert all(len(set(q)) == 4 for q in quads.tolist())
    prob = dict(K=W["K"], p3dw=W["p3dw"], p2d=W["p2d"], max_err=(pw.SIGMA2[np.arange(N) % pw.LEVELS] * F(5.991)).astype(F), quads=quads,
                min_inliers=min_inl)
    pose, inl = pm.hypotheses_multi([prob])[0]
    counts = inl.sum(axis=1)
    refined = {}

    def refine(h):
        if h not in refined:
            refined[h] = pm.refine(prob, inl[h])
        return int(refined[h][1].sum())
    it = pm.IterateModel(N, min_inl, max_its)
    endings = []
    for k, (T, no_more, n_inliers, vb) in enumerate(got["calls"]):
        ans, want_no_more, h = it.iterate(max_its if case.protocol == 1 else 5, counts, refine)     # (an IndexError: the class drew too few)
        endings.append(ans)
        if case.protocol == 0:
            assert (no_more == 1) == want_no_more, k
        want_vb = np.zeros(case.nf, bool)
        if ans == "nothing":
            assert T is None and n_inliers == 0 and len(vb) == 0, k
            continue
        if ans == "refined":
            rp, rin = refined[h]
            want_T, want_n = pose16(rp["R"][0], rp["t"][0]), int(rin.sum())
            want_vb[case.kept[rin]] = True
        else:
            want_T, want_n = pose16(pose["R"][h], pose["t"][h]), int(counts[h])
            want_vb[case.kept[inl[h]]] = True
        assert T is not None and T.tobytes() == want_T.tobytes(), (k, ans, h)
        assert n_inliers == want_n and np.array_equal(vb, want_vb), (k, ans, h)
    assert it.iterations <= len(quads) < it.iterations + max(max_its, 5) + 1        # nothing was drawn that no block asked for
    return endings, it


def libc_randi(seed):
    """DUtils::Random::RandomInt(0, n - 1) on the C library's own rand() after srand(seed)."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    libc.rand.restype = ctypes.c_int
    return lambda n: int((float(libc.rand()) / (2147483647.0 + 1.0)) * n)


def draw_quads(N, H, randi):
    out = []
    for _ in range(H):
        avail = list(range(N))
        for _ in range(4):
            r = randi(len(avail))
            out.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    return np.array(out, np.int32).reshape(-1, 4)


CPU_CASES = {
    "n8_below_min": dict(W=dict(N=8, bad=0.0, noise=0.0), extra=1),
    "n10_equal_min": dict(W=dict(N=10, bad=0.0, noise=0.0), extra=2),
    "n20_clean": dict(W=dict(N=20, bad=0.0, noise=0.0), extra=3),
    "n40_wrong30": dict(W=dict(N=40, bad=0.3, noise=1.0), extra=3),
    "n60_wrong60": dict(W=dict(N=60, bad=0.6, noise=1.0), extra=2),
    "n30_all_wrong": dict(W=dict(N=30, bad=1.0, noise=1.0), extra=1),
    "n50_find": dict(W=dict(N=50, bad=0.3, noise=1.0), extra=2, protocol=1),
}


def make_case(name, spec, seed=900):
    seed += sum(map(ord, name))
    return Case(pw.world(seed=seed, H=1, **spec["W"]), seed, protocol=spec.get("protocol", 0), extra=spec["extra"])


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_class_below_the_threshold_takes_the_host_routine(tmp_path, name):
    case = make_case(name, CPU_CASES[name])
    N = len(case.kept)
    max_its, min_inl, _ = pm.parameters(N, **PARAMS)
    (got,) = run_driver(tmp_path, [case], seed=17, mode=0)
    assert max_its * N < run_driver.host_below and 5 * N < run_driver.host_below      # every block of the case took the host routine
    res = check_against_model(case, got)
    if N >= min_inl:
        # the drawing itself: take-and-swap on RandomInt's arithmetic over the C library's rand(), block after block in one stream
        assert got["quads"].tolist() == draw_quads(N, len(got["quads"]), libc_randi(17)).tolist()
        assert len(got["quads"]) > max_its                        # the calls after bNoMore drew continuation blocks
    if name == "n8_below_min":
        assert res is None
    if name == "n10_equal_min":
        assert max_its == 1 and "refined" not in res[0] and res[0][0] == "best"      # Refine: 10 > 10 is false; mBestTcw at bNoMore
    if name in ("n20_clean", "n40_wrong30"):
        # a success, the solver called again after it, and beyond mRansacMaxIts the carried record answers again
        assert res[0][0] == "refined" and res[0].count("refined") >= 2 and res[1].iterations > max_its
    if name == "n30_all_wrong":
        assert set(res[0]) == {"nothing"}


def test_class_under_asan_ubsan(tmp_path, monkeypatch):
    """The sanitized build of the class and its driver (host/Makefile `san`) on three cases that need no device: a report fails the run."""
    host = os.path.dirname(DRIVER)
    subprocess.check_call(["make", "-s", "-C", host, "test_pnp_san"], timeout=900)
    monkeypatch.setattr("test_pnp_solver_class.DRIVER", os.path.join(host, "test_pnp_san"))
    monkeypatch.setenv("ASAN_OPTIONS", "detect_leaks=1:abort_on_error=0:exitcode=99")
    monkeypatch.setenv("UBSAN_OPTIONS", "print_stacktrace=1:halt_on_error=1:exitcode=98")
    cases = [make_case(n, CPU_CASES[n]) for n in ("n8_below_min", "n40_wrong30", "n50_find")]
    for case, got in zip(cases, run_driver(tmp_path, cases, seed=5, mode=0)):
        check_against_model(case, got)


GPU_SPECS = [dict(N=100, bad=0.3, noise=1.0), dict(N=64, bad=0.0, noise=0.0), dict(N=300, bad=0.6, noise=1.0), dict(N=2000, bad=0.3, noise=1.0),
             dict(N=8, bad=0.0, noise=0.0), dict(N=130, bad=0.3, noise=0.0), dict(N=500, bad=0.6, noise=1.0), dict(N=90, bad=0.3, noise=1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_solvers", [1, 3, 8])
def test_prepare_evaluates_every_solver_in_one_call_on_the_device(tmp_path, n_solvers):
    import torch  # noqa: F401
    cases = [Case(pw.world(seed=950 + i, H=1, **GPU_SPECS[i]), 950 + i, protocol=1 if i == 2 else 0, extra=1) for i in range(n_solvers)]
    if n_solvers > 1:
        cases[1] = None                                            # a discarded candidate: vpPnPsolvers[i] stays null
    got = run_driver(tmp_path, cases, seed=23, mode=1)
    # Prepare draws for every solver before anything else happens in the process: ONE stream of rand(), solver after solver
    randi = libc_randi(23)
    work = 0
    for c, g in zip(cases, got):
        if c is None:
            assert g is None
            continue
        check_against_model(c, g)
        N = len(c.kept)
        max_its, min_inl, _ = pm.parameters(N, **PARAMS)
        if N >= min_inl:
            work += max_its * N
            assert g["quads"][:max_its].tolist() == draw_quads(N, max_its, randi).tolist()
    assert work >= run_driver.host_below                         # the Prepare call went to the device
    # each solver preparing itself on its first iterate: every one equals the model on ITS OWN quadruples (the device runtime draws from
    # the same rand() stream when it is first used, so only the first solver's first block is that of the run above)
    single = run_driver(tmp_path, cases, seed=23, mode=0)
    for k, (c, g, s) in enumerate(zip(cases, got, single)):
        if c is None:
            assert s is None
            continue
        check_against_model(c, s)
        if k == 0:
            max_its = pm.parameters(len(c.kept), **PARAMS)[0]
            assert g["quads"][:max_its].tolist() == s["quads"][:max_its].tolist()
