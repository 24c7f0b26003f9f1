"""GPU half of the boundary tests of the PnPsolver port: every boundary problem of tests/pnp_boundary_worlds.py through orbm_pnp_ransac
on the device, once per call and once all together, every hypothesis record, mask word, refined record and refined mask word byte for
byte against orbm_pnp_ransac_host.  A mismatch is reported by the groups and sides of the cases that differ; the expected bit of every
case is ALSO read from the device's own mask words, so that nothing passes because host and device are wrong together; the record
problems assert which hypotheses became records and how many of them the device refined.  The worlds are built and checked on the CPU
(tests/test_pnp_boundary_worlds.py)."""
import pytest

import pnp_boundary_worlds as pb
import pnp_worlds as pw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(device=0)
    yield mt
    mt.close()


def test_the_worlds_meet_their_conditions():
    print(pb.check_conditions()[0])


def judged(w, got, want):
    """Everything one device answer can have wrong: against the host routine, against the expected bits, against the expected records."""
    out = pb.differences(w, got, want) + pb.wrong_bits(w, got)
    if "expect" in w and [int(h) for h in got[2]["hyp"]] != w["expect"]:
        out.append("%s [%s]: records %s for %s" % (w["name"], w["side"], [int(h) for h in got[2]["hyp"]], w["expect"]))
    return out


def condensed(wrong):
    """The findings without their problems' names, counted: the groups and sides of the cases that differ (the whole list is printed)."""
    print("\n".join(wrong))
    kinds = {}
    for x in wrong:
        kind = x.split(": ", 1)[1]
        kind = "bits without a case" if kind.endswith("bits without a case") else kind.split(" hyp ")[0].split(" ref ")[0]
        kinds[kind] = kinds.get(kind, 0) + 1
    return sorted(kinds.items())


def test_pnp_boundaries_one_call_per_problem(matcher):
    import multi_orb_slam_amd as m
    wrong = []
    for w, want in zip(pb.problems(), pb.host_answers()):
        got, = matcher.pnp_ransac([pw.problem(m, w)])
        n_rec = len(want[2])
        assert matcher.last_pnp()[:2] == (1, 0), w["name"]                   # nothing takes the host path
        if matcher.last_pnp()[2:] != (min(n_rec, m.PNP_MAX_RECORDS), max(0, n_rec - m.PNP_MAX_RECORDS)):
            wrong.append("%s: %s records refined on the device and behind it, of %d" % (w["name"], matcher.last_pnp()[2:], n_rec))
        wrong += judged(w, got, want)
    assert not wrong, condensed(wrong)


def test_pnp_boundaries_in_one_batch(matcher):
    """All problems in as few calls as ORBM_PNP_MAX_BATCH allows: the first mask word of a problem is then the sum of the earlier
    problems' hypotheses x words, the first refined word ORBM_PNP_MAX_RECORDS x the earlier problems' words, and the refined probes on
    record slot >= 1 stand behind problems of another word count."""
    import multi_orb_slam_amd as m
    probs, answers = pb.problems(), pb.host_answers()
    wrong = []
    for k in range(0, len(probs), m.PNP_MAX_BATCH):
        part = probs[k:k + m.PNP_MAX_BATCH]
        got = matcher.pnp_ransac([pw.problem(m, w) for w in part])
        assert len(got) == len(part) and matcher.last_pnp()[:2] == (len(part), 0)
        n_rec = [len(a[2]) for a in answers[k:k + m.PNP_MAX_BATCH]]
        if matcher.last_pnp()[2:] != (sum(min(n, m.PNP_MAX_RECORDS) for n in n_rec), sum(max(0, n - m.PNP_MAX_RECORDS) for n in n_rec)):
            wrong.append("batch at %d: %s records refined on the device and behind it, of %s" % (k, matcher.last_pnp()[2:], n_rec))
        for w, g, want in zip(part, got, answers[k:k + m.PNP_MAX_BATCH]):
            wrong += judged(w, g, want)
    assert not wrong, condensed(wrong)
