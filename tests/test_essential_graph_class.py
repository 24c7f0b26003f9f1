"""Optimizer::OptimizeEssentialGraph (host/Optimizer.h, host/EssentialGraph.cc) through its driver host/test_essential_graph: a stand-in map
(the local BA's builder and file format, tests/test_local_ba_class.py) with a graph on top -- a spanning tree by mnId, loop edges
between the current and the loop keyframe, camera-1 covisibility lists with weights, CorrectedSim3 / NonCorrectedSim3, LoopConnections,
the points' mnCorrectedByKF / mnCorrectedReference -- against a transcription of steps 2-4 (src/Optimizer.cc:1414-1613) and 6-7
(:1620-1676) around the library's own call on the arrays the transcription makes: the values written by SetPose / SetWorldPos and the
ORDER of the calls on the map, the lock before the first SetPose included.  The driver keeps its keyframes in one vector, so the heap
order the function follows through LoopConnections and the sets is the order of the file.  The CPU half stays under EG_HOST_BELOW edges
(the class takes the host routine), the GPU half lies above it (the device)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import multi_orb_slam_amd as m
import gba_worlds as gw
import test_local_ba_class as lbc
from sim3opt_model import Sim3
from eg_worlds import rot_sim3, vec8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_essential_graph")
HOST_BELOW = int(re.search(r"const int EG_HOST_BELOW = (\d+);", open(os.path.join(HOST, "EssentialGraph.cc")).read()).group(1))
MIN_FEAT = 100


def own_sim3(Tcw):
    """Converter::toMatrix3d / toVector3d of the float pose, g2o::Sim3(Rcw, tcw, 1.0)"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return Sim3.from_matrix([[float(T[r, c]) for c in range(3)] for r in range(3)], [float(T[r, 3]) for r in range(3)], 1.0)


def make_graph(M, seed, fix_scale, dense=False):
    """The graph on top of the map M (lbc.make_map): everything by keyframe POSITION in M["kfs"]."""
    rng = np.random.RandomState(seed)
    kfs, mps = M["kfs"], M["mps"]
    n = len(kfs)
    by_id = sorted(range(n), key=lambda i: kfs[i]["id"])
    good = [i for i in by_id if not kfs[i]["bad"]]
    loop, cur = good[0], good[-1]
    parent = {i: -1 for i in range(n)}
    children = {i: [] for i in range(n)}
    for a, b in zip(by_id[:-1], by_id[1:]):
        parent[b] = a; children[a].append(b)
    loop_edges = {i: [] for i in range(n)}
    loop_edges[cur].append(loop); loop_edges[loop].append(cur)          # mnId on either side: only the larger one adds the edge
    B, Cn = good[-2], good[1] if len(good) > 3 else good[0]              # a neighbour of the current keyframe and a far one
    A = good[len(good) // 2]
    weight = {}                                                         # (i, j) -> GetWeight_cam1
    weight[(cur, loop)] = 20                                            # below minFeat: the exception for the current-loop pair
    weight[(cur, A)] = 150
    weight[(B, loop)] = 30                                              # below minFeat: skipped
    weight[(B, Cn)] = 120                                               # added: the pair is in sInsertedEdges for step 4.3
    connections = {cur: sorted({loop, A} - {cur}), B: sorted({loop, Cn} - {B})}
    cov = {i: [] for i in range(n)}
    for i in range(n):
        others = [j for j in range(n) if j != i and (dense or rng.uniform() < 0.6)]
        for j in others:
            w = weight.get((i, j), weight.get((j, i), int(rng.randint(60, 200))))
            weight.setdefault((i, j), w)
            cov[i].append((j, weight[(i, j)]))
        cov[i].sort(key=lambda c: -c[1])
    for (i, j) in ((cur, loop), (cur, A), (B, loop), (B, Cn)):          # the pairs of LoopConnections have their weights in the lists
        if i != j and j not in [c[0] for c in cov[i]]:
            cov[i].append((j, weight[(i, j)])); cov[i].sort(key=lambda c: -c[1])
    corrected, non_corrected = {}, {}
    for k, i in enumerate([cur, B]):                                    # the others are absent from CorrectedSim3
        own = own_sim3(kfs[i]["Tcw"])
        fix = rot_sim3([0.3, 1.0, -0.2], 0.01 * (k + 1), [0.02, -0.01, 0.03 * (k + 1)], 1.0 if fix_scale else 1.0 + 0.02 * (k + 1))
        corrected[i] = fix * own
        non_corrected[i] = own
    bad = [i for i in range(n) if kfs[i]["bad"]]
    points = []
    for l, P in enumerate(mps):
        if l % 3 == 0:
            ref = bad[0] if (bad and l % 6 == 0) else by_id[(l * 7) % n]
            points.append((kfs[cur]["id"], kfs[ref]["id"]))             # corrected by pCurKF: nIDr = mnCorrectedReference
        else:
            points.append((0 if kfs[cur]["id"] != 0 else 999, 0))
    return {"loop": loop, "current": cur, "fix_scale": int(fix_scale), "max_id": max(K["id"] for K in kfs), "parent": parent,
            "children": children, "loop_edges": loop_edges, "cov": cov, "weight": weight, "corrected": corrected,
            "non_corrected": non_corrected, "connections": connections, "points": points}


def hd(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def write_graph(M, G, path):
    n = len(M["kfs"])
    out = ["%d %d %d %d" % (G["loop"], G["current"], G["fix_scale"], G["max_id"])]
    for i in range(n):
        out.append("%d %d %s %d %s %d %s" % (G["parent"][i], len(G["children"][i]), " ".join(map(str, G["children"][i])),
                                             len(G["loop_edges"][i]), " ".join(map(str, G["loop_edges"][i])), len(G["cov"][i]),
                                             " ".join("%d %d" % c for c in G["cov"][i])))
    for poses in (G["corrected"], G["non_corrected"]):
        out.append("%d" % len(poses))
        for i in sorted(poses):
            out.append("%d %s" % (i, " ".join(hd(v) for v in vec8(poses[i]))))
    out.append("%d" % len(G["connections"]))
    for i in sorted(G["connections"]):
        out.append("%d %d %s" % (i, len(G["connections"][i]), " ".join(map(str, G["connections"][i]))))
    for by, ref in G["points"]:
        out.append("%d %d" % (by, ref))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def transcription(M, G, run):
    kfs, mps = M["kfs"], M["mps"]
    n = len(kfs)
    ident = lambda: Sim3([0., 0., 0., 1.], [0., 0., 0.], 1.)
    id_of = [K["id"] for K in kfs]
    vScw = {}
    for i in range(n):                                                   # step 2
        if kfs[i]["bad"]:
            continue
        vScw[id_of[i]] = G["corrected"][i] if i in G["corrected"] else own_sim3(kfs[i]["Tcw"])
    scw = lambda ident_id: vScw.get(ident_id, ident())
    free = sorted([i for i in range(n) if not kfs[i]["bad"] and i != G["loop"]], key=lambda i: id_of[i])
    verts = free + ([G["loop"]] if not kfs[G["loop"]]["bad"] else [])
    vertex_of = {i: v for v, i in enumerate(verts)}
    ev0, ev1, meas, inserted = [], [], [], set()
    loop_id, cur_id = id_of[G["loop"]], id_of[G["current"]]

    def add(i, j, S):
        if i not in vertex_of or j not in vertex_of:
            return False
        ev0.append(vertex_of[i]); ev1.append(vertex_of[j]); meas.append(vec8(S))
        return True

    def w_cam1(i, j):
        return dict(G["cov"][i]).get(j, 0)

    for i in sorted(G["connections"]):                                   # step 3 (heap order = position)
        Swi = scw(id_of[i]).inverse()
        for j in G["connections"][i]:
            if (id_of[i] != cur_id or id_of[j] != loop_id) and w_cam1(i, j) < MIN_FEAT:
                continue
            if add(i, j, scw(id_of[j]) * Swi):
                inserted.add((min(id_of[i], id_of[j]), max(id_of[i], id_of[j])))
    non = lambda j: G["non_corrected"][j] if j in G["non_corrected"] else scw(id_of[j])
    for i in range(n):                                                   # step 4, vpKFs' order, bad keyframes included
        Swi = non(i).inverse()
        p = G["parent"][i]
        if p >= 0:
            add(i, p, non(p) * Swi)
        for l in sorted(G["loop_edges"][i]):
            if id_of[l] < id_of[i]:
                add(i, l, non(l) * Swi)
        covis = G["cov"][i]
        k = 0
        while k < len(covis) and not (MIN_FEAT > covis[k][1]):
            k += 1
        if not covis or k == len(covis):                                 # upper_bound found nothing below minFeat: an empty vector
            covis_sel = []
        else:
            covis_sel = [c[0] for c in covis[:k]]
        for j in covis_sel:
            if j != p and j not in G["children"][i] and j not in G["loop_edges"][i]:
                if not kfs[j]["bad"] and id_of[j] < id_of[i]:
                    if (min(id_of[i], id_of[j]), max(id_of[i], id_of[j])) in inserted:
                        continue
                    add(i, j, non(j) * Swi)
    rows, pts, refs = {}, [], []
    pos_of_id = {id_of[i]: i for i in range(n)}
    for l, P in enumerate(mps):                                          # step 7's inputs
        if P["bad"]:
            continue
        by, cref = G["points"][l]
        nIDr = cref if by == cur_id else id_of[P["ref"]]
        rows[l] = len(pts)
        pts.append(P["pos"]); refs.append(vertex_of.get(pos_of_id.get(nIDr, -1), -1))
    vertex = np.array([vec8(scw(id_of[i])) for i in verts]).reshape(-1, 8)
    P = m.EssentialGraphProblem(len(free), vertex, np.array(meas).reshape(-1, 8), ev0, ev1, np.array(pts, np.float32).reshape(-1, 3), refs,
                                bool(G["fix_scale"]))
    R = run(P)
    want_kf, want_mp, calls = [], [], [("lock", 0, 0)]
    for i, K in enumerate(kfs):
        pose = np.asarray(K["Tcw"], np.float32)
        if i in vertex_of:
            pose = R.Tiw[vertex_of[i]]; calls.append(("SetPose", K["id"], 0))
        want_kf.append((K["id"], pose.tobytes()))
    for l, Pt in enumerate(mps):
        pos = np.asarray(Pt["pos"], np.float32)
        if l in rows:
            pos = R.point_f[rows[l]]; calls.append(("SetWorldPos", Pt["id"], 0))
        want_mp.append((Pt["id"], pos.tobytes()))
    calls += [("SetNormalAndDepth", mps[l]["id"], 0) for l in range(len(mps)) if l in rows]
    calls.append(("unlock", 0, 0))
    return want_kf, want_mp, calls, R, P


def drive(M, G, tmp_path, driver=DRIVER, env=None):
    mp, gp = str(tmp_path / "map.txt"), str(tmp_path / "graph.txt")
    lbc.write_map(M, mp)
    write_graph(M, G, gp)
    out = subprocess.run([driver, mp, gp], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got_kf, got_mp, got_calls = [], [], []
    bits = lambda t: np.array([int(v, 16) for v in t], np.uint32).view(np.float32).tobytes()
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "KF":
            got_kf.append((int(t[1]), bits(t[2:18])))
        elif t[0] == "MP":
            got_mp.append((int(t[1]), bits(t[2:5])))
        elif t[0] == "CALL":
            got_calls.append((t[1], int(t[2]), int(t[3])))
    return got_kf, got_mp, got_calls, out.stdout + out.stderr


def check(M, G, tmp_path, run, **kw):
    want_kf, want_mp, want_calls, R, P = transcription(M, G, run)
    got_kf, got_mp, got_calls, _ = drive(M, G, tmp_path, **kw)
    assert len(got_kf) == len(want_kf) and len(got_mp) == len(want_mp)
    for g, w in zip(got_kf, want_kf):
        assert g == w, ("keyframe", g[0], w[0])
    for g, w in zip(got_mp, want_mp):
        assert g == w, ("point", g[0], w[0])
    first_diff = next((k for k, (g, w) in enumerate(zip(got_calls, want_calls)) if g != w), None)
    assert first_diff is None and len(got_calls) == len(want_calls), (first_diff, len(got_calls), len(want_calls),
                                                                        got_calls[first_diff or 0:(first_diff or 0) + 3], want_calls[first_diff or 0:(first_diff or 0) + 3])
    return R, P, want_calls


def host_route(P):
    assert P.n_edges < HOST_BELOW
    return m.essential_graph_host(P, 20, m.POSE_ORDER_DEVICE)


def small_map(bad_kf):
    # 15 points: fewer than REFRESH_HOST_BELOW (16), so that RefreshMapPoints too takes its host routine
    return lbc.make_map(gw.make_world(7, 15, 61, "mixed", 0.1, 4, True, "off"), 5, bad_kf=bad_kf)


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("bad_kf", [False, True])
def test_the_class_on_the_host_route(bad_kf, fix_scale, tmp_path):
    M = small_map(bad_kf)
    G = make_graph(M, 9, fix_scale)
    R, P, calls = check(M, G, tmp_path, host_route)
    kfs = M["kfs"]
    n_good = sum(1 for K in kfs if not K["bad"])
    assert P.n_vertices == n_good and P.n_free == n_good - 1 and R.optimised == 1 and R.round["iterations"][0] >= 1
    kinds = [c[0] for c in calls]
    assert kinds[0] == "lock" and kinds[-1] == "unlock" and kinds.count("SetPose") == n_good        # the lock before the first SetPose
    assert kinds.count("SetWorldPos") == kinds.count("SetNormalAndDepth") == P.n_points > 0
    assert kinds.index("SetWorldPos") > max(k for k, v in enumerate(kinds) if v == "SetPose")
    # the cases the graph was built for
    pair = lambda a, b: any(P.edge_v0[e] == a and P.edge_v1[e] == b for e in range(P.n_edges))
    free = sorted([i for i in range(len(kfs)) if not kfs[i]["bad"] and i != G["loop"]], key=lambda i: kfs[i]["id"])
    v = {i: k for k, i in enumerate(free + [G["loop"]])}
    cur, loop = G["current"], G["loop"]
    assert G["weight"][(cur, loop)] < MIN_FEAT and pair(v[cur], v[loop])                      # the current-loop pair below minFeat
    B = sorted(G["connections"])[0] if sorted(G["connections"])[0] != cur else sorted(G["connections"])[1]
    assert not any(P.edge_v0[e] == v[B] and P.edge_v1[e] == v[loop] for e in range(P.n_edges)) or G["parent"][B] == loop   # 30 < minFeat
    assert sum(1 for i in range(len(kfs)) if i not in G["corrected"] and not kfs[i]["bad"]) > 0  # keyframes absent from CorrectedSim3
    assert (np.asarray(P.point_ref) == -1).any() == bad_kf                                      # a reference keyframe without a vertex
    by = [p[0] for p in G["points"]]
    assert kfs[cur]["id"] in by and any(b != kfs[cur]["id"] for b in by)                        # corrected by pCurKF and not
    if bad_kf:
        assert P.n_vertices < len(kfs)


def test_a_covisible_pair_already_inserted_is_not_added_again(tmp_path):
    M = small_map(False)
    G = make_graph(M, 9, False)
    _, P, _ = check(M, G, tmp_path, host_route)
    G2 = dict(G, connections={k: v for k, v in G["connections"].items() if k == G["current"]})   # without B's loop connections
    _, P2, _ = check(M, G2, tmp_path, host_route)
    # B - C came from LoopConnections once; without that entry step 4.3 adds it itself (or the count drops by the one edge)
    assert P2.n_edges in (P.n_edges, P.n_edges - 1)
    kfs = M["kfs"]
    ids = lambda Pq: sorted((min(a, b), max(a, b)) for a, b in zip(Pq.edge_v0, Pq.edge_v1))
    assert all(ids(P).count(p) <= 2 for p in ids(P))


def test_the_class_under_asan_and_ubsan(tmp_path):
    """The sanitized stand-alone driver (host/Makefile: test_essential_graph_san) on the host route; the same answers."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_essential_graph_san"], timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    for bad_kf, fix_scale in ((False, False), (True, True)):
        M = small_map(bad_kf)
        G = make_graph(M, 9, fix_scale)
        check(M, G, tmp_path, host_route, driver=DRIVER + "_san", env=env)
        out = drive(M, G, tmp_path, driver=DRIVER + "_san", env=env)[3]
        assert not any(mk in out for mk in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))


@pytest.mark.gpu
def test_the_class_on_the_device(tmp_path):
    W = gw.make_world(40, 120, 62, "mixed", 0.1, 6, True, "off")
    mt = m.Matcher(0.8, True)
    try:
        def device_route(P):
            assert P.n_edges >= HOST_BELOW
            R = mt.essential_graph(P, 20)
            assert mt.last_essential_graph()[0] == 0
            return R
        for fix_scale in (False, True):
            M = lbc.make_map(W, 6)
            G = make_graph(M, 10, fix_scale, dense=True)
            R, P, calls = check(M, G, tmp_path, device_route)
            assert R.optimised == 1 and P.n_free == len(M["kfs"]) - 1 and len(calls) > 100
    finally:
        mt.close()
