"""k_db_query on the MI355X held to the boundary worlds of tests/kfdb_boundary_worlds.py: KeyFrameDatabase.query and .score against the
model on keys, common counts and every score's bytes -- every query alone and inside one batched call -- and the launch each call made
(form, entries per workgroup, workgroups, queries: KeyFrameDatabase.last_query()) against the one derived from run_query's arithmetic, so
that no test passes without running the form it names.  The worlds' conditions and the wrong rules are asserted on the CPU in
tests/test_kfdb_boundary_worlds.py."""
import functools
import pytest
import multi_orb_slam_amd as m
import kfdb_boundary_worlds as kw

pytestmark = pytest.mark.gpu

WORLDS = {w["name"]: w for w in kw.worlds()}


@functools.lru_cache(None)
def transcripts(name):
    w = WORLDS[name]
    db = m.KeyFrameDatabase(w["n_words"])
    got = kw.play(w, db, refusal=m.OrbError)
    db.close()
    return got, kw.play(w, kw.ModelDB(w["n_words"]))


def test_no_world_is_left_out():
    assert len(WORLDS) == kw.N_WORLDS and {w["group"] for w in WORLDS.values()} == set(kw.GROUPS)


@pytest.mark.parametrize("name", list(WORLDS))
def test_query_and_score_equal_the_model_byte_for_byte(name):
    got, want = transcripts(name)
    assert kw.differences(got, want) == []
    assert sum(len(r["batch"]) for k, r in got if k == "query") > 0


def launches(name):
    got, _ = transcripts(name)
    return [r["batch_launch"] for k, r in got if k == "query"], [l for k, r in got if k == "query" for l in r["alone_launch"]]


def test_both_forms_ran_at_the_switch():
    batch, alone = launches("switch")
    assert [b[0] for b in batch] == [m.vocabulary.DB_FORM_LDS] + [m.vocabulary.DB_FORM_GLOBAL] * 3 + [m.vocabulary.DB_FORM_LDS]
    assert {a[0] for a in alone} == {m.vocabulary.DB_FORM_LDS, m.vocabulary.DB_FORM_GLOBAL}
    got, _ = transcripts("switch")
    assert [r for k, r in got if k == "refused"] == [True, True]


def test_every_entries_per_workgroup_ran_with_full_and_partial_last_workgroups():
    batch, _ = launches("grid")
    epbs = {b[1] for b in batch}
    assert epbs == set(range(4, 65))
    assert {b[3] for b in batch} >= {1, 2, 3, 5, 1023, 1024}
    E_of = [r["entries"] for k, r in transcripts("grid")[0] if k == "query"]
    partial = [(b, E) for b, E in zip(batch, E_of) if E % b[1] == 1 and b[2] >= 2]
    exact = [(b, E) for b, E in zip(batch, E_of) if E == b[1]]
    assert len(partial) >= 60 and len(exact) >= 60
    assert [r for k, r in transcripts("grid")[0] if k == "refused"] == [True]


@pytest.mark.parametrize("name", ["chunk", "search", "values", "order"])
def test_the_small_worlds_ran_from_lds(name):
    batch, alone = launches(name)
    assert {b[0] for b in batch + alone} == {m.vocabulary.DB_FORM_LDS} and {b[1] for b in batch + alone} == {4}
