"""The keyframe database without a GPU: known answers of the checker (tests/kfdb_model.py), non-vacuity of the fixtures the GPU tests use,
the host restatement in the driver (`test_kfdb cpu`) against the checker, and what can be said about the build: exported signatures, the
reference's headers, the kernels' denormal mode."""
import os
import re
import struct
import subprocess
import numpy as np
import pytest
import multi_orb_slam_amd as m
import kfdb_model as km
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_kfdb")
REF = "/root/reference"
HAVE_REF = os.path.isdir(os.path.join(REF, "include"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present")
F32 = np.float32


B = km.B


def db_with(kfs, n_words=1000):
    db = km.ModelDatabase(n_words)
    for k in kfs:
        db.add(k); db.add_cam1(k)
    return db


# ------------------------------------------------------------------------------------------------------------ known answers
def test_empty_database_and_no_shared_word():
    q = km.KF(9, B(range(10)))
    assert km.ModelDatabase(100).detect_loop(q, 0.0)[0] == []
    assert km.ModelDatabase(100).detect_reloc(km.FrameOf(3, q))[0] == []
    db = db_with([km.KF(1, B(range(20, 30))), km.KF(2, B(range(40, 45)))])
    ids, tr = db.detect_loop(q, 0.0)
    assert ids == [] and tr["sharing"] == [] and tr["met"] == []
    assert db.detect_reloc(km.FrameOf(3, q))[0] == []


def test_everything_connected_gives_nothing_and_counts_one():
    a, b = km.KF(1, B(range(0, 6))), km.KF(2, B(range(3, 12)))
    q = km.KF(9, B(range(10)), conn=[a, b])
    db = db_with([a, b])
    ids, tr = db.detect_loop(q, 0.0)
    assert ids == [] and tr["sharing"] == [] and tr["met"] == [1, 2] and tr["raw_common"] == {1: 6, 2: 7}
    assert (a.mnLoopQuery, a.mnLoopWords, b.mnLoopQuery, b.mnLoopWords) == (0, 1, 0, 1)     # restarted at every meeting, never marked
    # camera 1 has its own connected set (empty here): both are listed
    assert db.detect_loop(q, 0.0, cam1=True)[1]["sharing"] == [1, 2]


def test_min_common_words_truncates_like_int_times_float():
    q = km.KF(9, B(range(10)))
    a, b, c = km.KF(1, B(list(range(0, 5)) + [20, 21])), km.KF(2, B(list(range(0, 4)) + [30])), km.KF(3, B([0, 1, 2, 40]))
    _, tr = db_with([a, b, c]).detect_loop(q, 0.0)
    assert tr["common"] == {1: 5, 2: 4, 3: 3} and tr["min_common"] == 4 and set(tr["scored"]) == {1}       # 5 * 0.8f -> 4
    q2 = km.KF(10, B(range(10)))
    b2, c2, d2 = km.KF(2, B(list(range(0, 4)) + [30])), km.KF(3, B([0, 1, 2, 40])), km.KF(4, B([1, 2, 3, 5, 50][:4]))
    _, tr = db_with([b2, c2, d2]).detect_loop(q2, 0.0)
    assert tr["common"] == {2: 4, 3: 3, 4: 4} and tr["min_common"] == 3 and set(tr["scored"]) == {2, 4}    # 4 * 0.8f -> 3
    assert b2.mLoopScore != 0 and c2.mLoopScore == 0 and c2.mnLoopQuery == 10                               # listed, not scored


def test_min_score_boundary_is_inclusive_in_float():
    a = km.KF(1, B(range(0, 7)))
    q = km.KF(9, B(range(10)))
    d = oracle.bow_score_l1(q.bow, a.bow)
    si = F32(d)
    assert float(si) != d      # the double does not survive the float: the comparison is made on the float
    ids, tr = db_with([a]).detect_loop(q, si)
    assert ids == [1] and tr["matches"] == [(float(si), 1)]
    a2 = km.KF(1, B(range(0, 7)))
    ids, tr = db_with([a2]).detect_loop(km.KF(10, B(range(10))), np.nextafter(si, F32(2), dtype=F32))
    assert ids == [] and tr["matches"] == [] and set(tr["scored"]) == {1} and a2.mLoopScore == si


def test_group_best_is_a_neighbour_and_a_keyframe_best_in_two_groups_is_returned_once():
    a, b = km.KF(1, B(list(range(0, 8)) + [20, 21, 22, 23])), km.KF(2, B(range(0, 9)))
    a.cov, b.cov = [b], [a]
    q = km.KF(9, B(range(10)))
    ids, tr = db_with([a, b]).detect_loop(q, 0.0)
    sa, sb = F32(tr["scored"][1]), F32(tr["scored"][2])
    assert sb > sa
    assert tr["groups"] == [(float(F32(sa + sb)), 2, 1), (float(F32(sb + sa)), 2, 2)]
    assert ids == [2]
    # relocalisation: the same through the camera-1 lists
    a.cov1, b.cov1 = [b], [a]
    ids, tr = db_with([a, b]).detect_reloc(km.FrameOf(5, q))
    assert ids == [2] and [g[1:] for g in tr["groups"]] == [(2, 1), (2, 2)]


def test_erase_then_add_again_changes_the_order():
    a, b = km.KF(1, B(range(0, 6))), km.KF(2, B(range(0, 7)))
    db = db_with([a, b])
    assert db.detect_loop(km.KF(9, B(range(10))), 0.0)[1]["sharing"] == [1, 2]
    db.erase(a); db.add(a)
    assert db.detect_loop(km.KF(10, B(range(10))), 0.0)[1]["sharing"] == [2, 1]
    assert db.detect_reloc(km.FrameOf(5, km.KF(0, B(range(10)))))[1]["sharing"] == [2]      # erase took it out of both files
    db.erase(km.KF(77, B([1, 2])))                                                         # never added: nothing happens
    assert db.detect_loop(km.KF(11, B(range(10))), 0.0)[1]["sharing"] == [2, 1]


def test_scratch_field_quirks_of_the_reference():
    c = km.quirk_cases()
    r = km.run_script(*c["twice"])
    assert r[0][1] == [2] and r[0][2]["sharing"] == [1, 2, 3]
    assert r[1][1] == [] and r[1][2]["sharing"] == [] and r[1][2]["met"] == [1, 2, 3]
    assert [f[1] for f in r[0][3][:3]] == [6, 8, 5] and [f[1] for f in r[1][3][:3]] == [12, 16, 10]          # counted on top
    assert r[2][1] == [] and [f[1] for f in r[2][3][:3]] == [18, 24, 15]                                      # the camera-1 walk shares the fields
    r = km.run_script(*c["zero"])
    assert r[0][1] == [] and r[0][2]["sharing"] == [] and [f[:2] for f in r[0][3][1:4]] == [(0, 8), (0, 9), (0, 7)]
    assert r[1][2]["sharing"] == [1, 2, 3] and r[1][1] != []
    assert r[2][2]["sharing"] == [1, 3, 2] and r[2][1] != []                                                  # 2 was erased and added again
    assert r[3][1] == [] and r[3][2]["sharing"] == [] and [f[3:5] for f in r[3][3][1:4]] == [(0, 8), (0, 9), (0, 7)]
    r = km.run_script(*c["connected"])
    assert r[0][2]["sharing"] == [3] and r[0][1] == [3] and [f[:2] for f in r[0][3][:2]] == [(0, 1), (0, 1)]
    assert r[0][2]["groups"] == [(r[0][2]["matches"][0][0], 3, 3)]
    # camera 1: nothing connected, so 1 and 2 are listed; 3 carries the id from the call before and is counted on top instead
    assert r[1][2]["sharing"] == [1, 2] and r[1][3][2][:2] == (9, 16)
    r = km.run_script(*c["stale"])
    s5 = r[0][3][1][5]
    assert r[0][1] == [2] and s5 > 0
    assert r[1][2]["sharing"] == [1, 2] and set(r[1][2]["scored"]) == {1}
    assert r[1][3][1][3:] == (6, 3, s5)                                                                       # marked by frame 6, score of frame 5
    assert r[1][1] == [2] and r[1][2]["groups"][0][1:] == (2, 1)
    assert r[2][1] == [] and r[2][3][0][4] == 16                                                              # same frame id again


# ------------------------------------------------------------------------------------------- non-vacuity of the GPU fixtures
def test_generated_worlds_exercise_what_the_gpu_tests_compare():
    calls, in_add_order = [], []
    for K in (120, 400):
        w = km.World(K, seed=K)
        ops = w.script()
        # add sequence of every keyframe per file: the position of its LAST add in the script (all adds come before the first detect call;
        # a keyframe that was erased and added again takes its place behind the others, as in the reference's lists and in the device database)
        seq = {"add": {}, "add_cam1": {}}
        for i, (name, t, _, _) in enumerate(ops):
            if name in seq:
                seq[name][w.kfs[t].mnId] = i
        for name, ids, tr, fields in km.run_script(w.n_words, w.kfs, ops):
            calls.append((name, ids, tr, fields))
            order = seq["add" if name == "loop" else "add_cam1"]
            in_add_order.append(tr["sharing"] == sorted(tr["sharing"], key=order.__getitem__))
    assert len(calls) >= 30
    assert all(len(tr["sharing"]) >= 10 for _, _, tr, _ in calls)
    assert any(len(ids) >= 3 for _, ids, _, _ in calls)
    assert any(tr["sharing"] and not tr["matches"] for _, _, tr, _ in calls)                 # nothing reaches stage 3's list
    assert not all(in_add_order)                               # sharing order != ascending add sequence
    assert any(best != seed for _, _, tr, _ in calls for _, best, seed in tr["groups"])
    assert any(len(set(tr["first_word"].values())) < len(tr["first_word"]) for _, _, tr, _ in calls)     # the sequence tie-break decides
    # and id order would be the wrong tie-break: some keyframe that was added again is met at a word a keyframe with a larger id shares
    assert any(tr["met"] != [i for _, i in sorted((tr["first_word"][i], i) for i in tr["met"])] for _, _, tr, _ in calls)


@pytest.mark.parametrize("K", [2000, 10000])
def test_large_worlds_of_the_query_test_list_enough(K):
    w = km.World(K, seed=K)
    lap = K // 2
    asking = [w.kfs[lap + (j * 37 + 11) % (lap - 10)] for j in range(6)]
    db = km.ModelDatabase(w.n_words)
    for k in w.kfs:
        if k not in asking:
            db.add_cam1(k)
    for i, q in enumerate(asking):
        _, tr = db.detect_reloc(km.FrameOf(10 ** 9 + i, q))
        assert len(tr["sharing"]) >= 10 and len(tr["scored"]) >= 2 and tr["sharing"] != sorted(tr["sharing"])


# ------------------------------------------------------------------------------------------------------------ the product
def device_present():
    """Asked of the library itself: an existing handle constructor either works or reports ORB_E_NO_DEVICE (tests/test_abi.py)."""
    try:
        m.Matcher()
    except m.OrbError as e:
        assert e.code == -4
        return False
    return True


def test_no_device_is_a_loud_error():
    if device_present():
        assert len(m.KeyFrameDatabase(1000)) == 0
        return
    with pytest.raises(m.OrbError) as e:
        m.KeyFrameDatabase(1000)
    assert e.value.code == -4 and "no CPU path" in str(e.value)


def test_host_library_exports_the_reference_signatures():
    out = subprocess.run(["nm", "-DC", os.path.join(ROOT, "multi_orb_slam_amd", "lib", "libmorb_host.so")], capture_output=True, text=True, check=True).stdout
    for sig in ("KeyFrameDatabase::KeyFrameDatabase(ORB_SLAM2::ORBVocabulary const&)", "KeyFrameDatabase::add(ORB_SLAM2::KeyFrame*)",
                "KeyFrameDatabase::add_cam1(ORB_SLAM2::KeyFrame*)", "KeyFrameDatabase::erase(ORB_SLAM2::KeyFrame*)", "KeyFrameDatabase::clear()",
                "KeyFrameDatabase::DetectLoopCandidates(ORB_SLAM2::KeyFrame*, float)",
                "KeyFrameDatabase::DetectLoopCandidates_cam1(ORB_SLAM2::KeyFrame*, float)",
                "KeyFrameDatabase::DetectRelocalizationCandidates(ORB_SLAM2::Frame*)"):
        assert re.search(r" T ORB_SLAM2::" + re.escape(sig), out), sig


def run_cpu(tmp_path, name, n_words, kfs, ops):
    world, out = tmp_path / (name + ".bin"), tmp_path / (name + "_cpu.bin")
    km.write_world(world, n_words, kfs, ops)
    exp = km.expected_out(km.run_script(n_words, kfs, ops))
    r = subprocess.run([DRIVER, "cpu", str(world), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = km.read_out(out, len(kfs))
    assert len(got) == len(exp) > 0
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g[0] == e[0], (name, i, g[0], e[0])
        assert g[1] == e[1], (name, i)
    return exp


def test_host_restatement_equals_the_model_on_the_quirks(tmp_path):
    for name, case in km.quirk_cases().items():
        run_cpu(tmp_path, name, *case)


@pytest.mark.parametrize("K", [120, 400])
def test_host_restatement_equals_the_model_on_generated_worlds(tmp_path, K):
    w = km.World(K, seed=K)
    exp = run_cpu(tmp_path, "world%d" % K, w.n_words, w.kfs, w.script())
    assert max(len(ids) for ids, _ in exp) >= 2


def test_query_kernels_keep_f64_denormals_and_hold_no_packed_f32(tmp_path):
    import test_isa_guard as guard
    seen = 0
    for co in guard.code_objects(m.LIB_PATH):
        for name, kd in guard.kernel_descriptors(co).items():
            if "k_db_query" in name:
                rsrc1, = struct.unpack_from("<I", kd, 48)
                assert (rsrc1 >> 18) & 3 == 3, (name, hex(rsrc1))     # FLOAT_DENORM_MODE_16_64: denormals in and out
                seen += 1
    assert seen >= 2      # the LDS form and the general form
    if not os.path.exists(guard.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    kernels = {k: v for k, v in guard.disassemble(tmp_path).items() if "k_db_query" in k}
    assert len(kernels) >= 2
    for name, ins in kernels.items():
        assert not [i for i in ins if re.search(r"\bv_pk_\w+_f32\b", i)], name
        assert not [i for i in ins if re.match(r"v_fma", i)], name                       # nothing to contract, and nothing contracted
        assert sum(i.startswith("v_add_f64") for i in ins) >= 3 and any(i.startswith("v_readlane_b32") for i in ins), name


# ---------------------------------------------------------------------------------------------------- the reference's headers
def _syntax_only(src, includes):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-ffp-contract=off", "-DMORB_USE_REFERENCE_TYPES"]
    for inc in includes:
        cmd += ["-I", inc]
    cmd.append(src)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return p.returncode, [ln for ln in p.stderr.splitlines() if "error" in ln]


@needs_ref
def test_class_compiles_against_the_reference_headers_in_place():
    rc, errors = _syntax_only(os.path.join(HOST, "KeyFrameDatabase.cc"),
                              [HOST, os.path.join(HOST, "cv_shim"), os.path.join(REF, "include"), REF, os.path.join(ROOT, "include")])
    assert rc == 0 and not errors, "\n".join(errors[:20])


def _replaced_tree(tmp_path):
    inc = tmp_path / "include"
    inc.mkdir()
    for name in os.listdir(os.path.join(REF, "include")):
        os.symlink(os.path.join(REF, "include", name), inc / name)
    for name in ("ORBextractor.h", "ORBmatcher.h", "ORBVocabulary.h", "KeyFrameDatabase.h"):      # ours take the place of the reference's four
        os.unlink(inc / name)
        os.symlink(os.path.join(HOST, name), inc / name)
    for name in ("cv_compat.h", "slam_types.h"):
        os.symlink(os.path.join(HOST, name), inc / name)
    return str(inc)


@needs_ref
@pytest.mark.parametrize("src", ["KeyFrameDatabase.cc", "ORBmatcher.cc", "ref:src/MapPoint.cc", "ref:src/Map.cc"])
def test_replaced_header_tree_with_our_database_header(tmp_path, src):
    inc = _replaced_tree(tmp_path)
    path = os.path.join(REF, src[4:]) if src.startswith("ref:") else os.path.join(HOST, src)
    rc, errors = _syntax_only(path, [inc, os.path.join(HOST, "cv_shim"), REF, os.path.join(ROOT, "include")])
    assert rc == 0 and not errors, "\n".join(errors[:20])
