"""The guidance-reuse plan (chronoedit_amd/guidance.py): a pure function of the schedule's length, the config and the forced pairs.  No GPU."""
import itertools
import math

import pytest

from chronoedit_amd.guidance import GuidanceReuseConfig, plan, rel_l2_from_sums, report

P, R, O = "pair", "reuse", "off"


def test_hand_written_plans():
    assert plan(6, GuidanceReuseConfig(pair_every=2)) == [P, R, P, R, P, R]
    assert plan(8, GuidanceReuseConfig(pair_every=3, interval=(0.25, 0.75))) == [O, O, P, R, R, P, O, O]
    assert plan(7, GuidanceReuseConfig(pair_every=3)) == [P, R, R, P, R, R, P]
    assert plan(0, GuidanceReuseConfig()) == []
    assert GuidanceReuseConfig() == GuidanceReuseConfig(pair_every=2, interval=(0.0, 1.0))


def test_a_forced_pair_restarts_the_count():
    cfg = GuidanceReuseConfig(pair_every=3)
    assert plan(8, cfg) == [P, R, R, P, R, R, P, R]
    assert plan(8, cfg, forced_pairs={2}) == [P, R, P, R, R, P, R, R]
    assert plan(8, cfg, forced_pairs=(1, 2)) == [P, P, P, R, R, P, R, R]
    assert plan(8, cfg, forced_pairs={3}) == plan(8, cfg)  # already a pair
    # a forced index outside the interval stays "off"; one inside still restarts
    inner = GuidanceReuseConfig(pair_every=3, interval=(0.25, 0.75))
    assert plan(8, inner, forced_pairs={0, 7}) == [O, O, P, R, R, P, O, O]
    assert plan(8, inner, forced_pairs={3}) == [O, O, P, P, R, R, O, O]
    assert plan(8, inner, forced_pairs={99, -1}) == plan(8, inner)


def test_pair_every_one_and_the_empty_interval():
    for n in (1, 6, 50):
        assert plan(n, GuidanceReuseConfig(pair_every=1)) == [P] * n
        assert plan(n, GuidanceReuseConfig(pair_every=4, interval=(0, 0))) == [O] * n
        assert plan(n, GuidanceReuseConfig(pair_every=1, interval=(0.5, 0.5))) == [O] * n


@pytest.mark.parametrize("n, pe, interval", list(itertools.product((1, 5, 6, 50), (1, 2, 3, 7), ((0.0, 1.0), (0.0, 0.67), (0.2, 0.8), (0.3, 0.31), (1.0, 1.0)))))
def test_the_rules(n, pe, interval):
    lo, hi = interval
    forced = {2, n - 1}
    got = plan(n, GuidanceReuseConfig(pe, interval), forced)
    assert len(got) == n
    since = None
    for i, k in enumerate(got):
        inside = lo * n <= i < hi * n
        assert (k == O) == (not inside), (i, k)
        if not inside:
            since = None
            continue
        if since is None:
            assert k == P, f"step {i}: the first inside step (after an off run) is a pair"
        if i in forced:
            assert k == P, f"step {i} is forced"
        if k == P:
            assert since is None or since == pe or i in forced, f"step {i}: a pair before the count ran out"
            since = 1
        else:
            assert since < pe, f"step {i}: more than pair_every - 1 reuse steps after a pair"
            since += 1
    rep = report(got)
    assert rep["plan"] == got and rep["pair"] + rep["reuse"] + rep["off"] == n
    assert set(rep) == {"plan", "pair", "reuse", "off"}
    assert rep["pair"] == got.count(P) and rep["reuse"] == got.count(R) and rep["off"] == got.count(O)


@pytest.mark.parametrize("kw", [dict(pair_every=0), dict(pair_every=-2), dict(pair_every=1.5), dict(interval=(-0.1, 1.0)), dict(interval=(0.0, 1.1)),
                                dict(interval=(0.6, 0.4)), dict(interval=(0.0, float("nan"))), dict(interval=(0.5,)), dict(interval=0.5)])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        plan(6, GuidanceReuseConfig(**kw))


def test_a_config_that_skipped_its_own_check_is_still_refused_by_plan():
    cfg = GuidanceReuseConfig()
    object.__setattr__(cfg, "pair_every", 0)
    with pytest.raises(ValueError):
        plan(6, cfg)


def test_rel_l2_from_sums_marks_missing_ages_nan():
    sums = [[float("nan"), float("nan"), 4.0], [1.0, 123.0, 4.0], [1.0, 9.0, 4.0], [0.0, 0.0, 0.0]]
    got = rel_l2_from_sums(sums, 2, history=[0, 1, 2, 2])
    assert all(math.isnan(v) for v in got[0])
    assert got[1][0] == 0.5 and math.isnan(got[1][1])
    assert got[2] == [0.5, 1.5]
    assert all(math.isnan(v) for v in got[3])  # an all-zero direction has no relative distance
