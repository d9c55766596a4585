"""Posteriors.plan_batched_calls: which blocks of a batch fitted together go through batched calls, and in which
sub-batches.  The planner is pure (region ids, bounds, byte counts), so its rules are checked here without a device; the
expected values are written out from the rules, or derived by ``_expected`` below, a second statement of them."""
import random

import pytest

from cimrgp_amd.Posteriors import plan_batched_calls

REGIONS = list(range(8))
BOUNDS = [(10 * l, 10 * l + 10) for l in range(7)] + [(70, 83)]          # region 7 takes the remainder


def _tens(lo, hi):
    return list(range(10 * lo, 10 * hi, 10))


TABLE = [
    # owned, bounds, per-block bytes, budget -> calls (i0, nb, ns, test start rows), covered
    ('one call', set(REGIONS), BOUNDS, lambda ns: 100 * ns, 10 ** 9, [(0, 7, 10, _tens(0, 7))], set(range(7))),
    ('memory-bounded split, trailing batch of one', set(REGIONS), BOUNDS, lambda ns: 100 * ns, 3000,
     [(0, 3, 10, [0, 10, 20]), (3, 3, 10, [30, 40, 50]), (6, 1, 10, [60])], set(range(7))),
    ('not contiguous', {0, 2, 4, 6}, BOUNDS, lambda ns: 1, 10 ** 9, [], set()),
    ('a run and a loner of another size', {2, 3, 4, 7}, BOUNDS, lambda ns: 1, 10 ** 9, [(2, 3, 10, [20, 30, 40])], {2, 3, 4}),
    ('training rows', {2, 3, 4}, None, lambda ns: 7, 20, [(2, 2, None, []), (4, 1, None, [])], {2, 3, 4}),
    ('no test points', set(REGIONS), [(5, 5)] * 8, lambda ns: 1, 10 ** 9, [], set()),
    ('two sizes, both contiguous', set(range(6)), [(0, 4), (4, 8), (8, 12), (12, 19), (19, 26), (26, 33)], lambda ns: ns, 10 ** 9,
     [(0, 3, 4, [0, 4, 8]), (3, 3, 7, [12, 19, 26])], set(range(6))),
    ('budget below one block', {1, 2, 3}, BOUNDS, lambda ns: 1000 * ns, 9999,
     [(1, 1, 10, [10]), (2, 1, 10, [20]), (3, 1, 10, [30])], {1, 2, 3}),
    ('float budget', set(REGIONS), BOUNDS, lambda ns: 100 * ns, 0.5 * 8001.0,
     [(0, 4, 10, _tens(0, 4)), (4, 3, 10, _tens(4, 7))], set(range(7))),
    ('a zero byte count divides as 1', {0, 1}, BOUNDS, lambda ns: 0, 1, [(0, 1, 10, [0]), (1, 1, 10, [10])], {0, 1}),
]


@pytest.mark.parametrize('name,owned,bounds,per_block,budget,calls,covered', TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(name, owned, bounds, per_block, budget, calls, covered):
    got_calls, got_covered = plan_batched_calls(REGIONS, owned, bounds, per_block, budget)
    assert sorted(got_calls) == calls
    assert got_covered == covered


def test_plan_indexes_the_arena_not_the_regions():
    """A batch holds the regions in the order they were fitted: (i0, nb) are positions in that order."""
    regions = [6, 5, 4, 9]
    calls, covered = plan_batched_calls(regions, {4, 5, 6}, BOUNDS, lambda ns: 1, 2)
    assert calls == [(0, 2, 10, [60, 50]), (2, 1, 10, [40])]
    assert covered == {4, 5, 6}
    calls, covered = plan_batched_calls(regions, {6, 4}, BOUNDS, lambda ns: 1, 2)        # positions 0 and 2: a gap
    assert (calls, covered) == ([], set())


def test_plan_asks_the_byte_count_per_group_size():
    seen = []

    def per_block(ns):
        seen.append(ns)
        return ns

    bounds = [(0, 4), (4, 8), (8, 15), (15, 22), (22, 22)]
    plan_batched_calls(list(range(5)), set(range(5)), bounds, per_block, 100)
    assert sorted(seen) == [4, 7]                    # not for the empty block, which is its own (skipped) group


def _expected(regions, owned, bounds, per_block, budget):
    """The rules, stated block by block: block i may be batched iff the owned blocks with its number of test points are
    at least 2, have test points, and sit at consecutive arena positions; such a run is cut from its start into
    sub-batches of max(1, budget // max(1, per_block(ns))) blocks (at most the run)."""
    pos = {l: i for i, l in enumerate(regions)}
    ns_of = (lambda l: None) if bounds is None else (lambda l: int(bounds[l][1]) - int(bounds[l][0]))
    groups = {}
    for l in regions:
        if l in owned:
            groups.setdefault(ns_of(l), []).append(l)
    calls, covered = [], set()
    for ns, members in groups.items():
        places = sorted(pos[l] for l in members)
        if len(members) < 2 or (ns is not None and ns <= 0) or places[-1] - places[0] != len(places) - 1:
            continue
        width = max(1, min(len(members), int(budget // max(1, per_block(ns)))))
        for p in range(places[0], places[-1] + 1, width):
            nb = min(width, places[-1] + 1 - p)
            calls.append((p, nb, ns, [] if bounds is None else [int(bounds[regions[i]][0]) for i in range(p, p + nb)]))
        covered.update(members)
    return sorted(calls, key=lambda c: c[0]), covered


def _random_case(rng):
    n = rng.randint(1, 12)
    regions = list(range(n))
    if rng.random() < 0.3:
        rng.shuffle(regions)
    if rng.random() < 0.5:                           # a rank's share: a range of regions
        lo = rng.randint(0, n - 1)
        owned = set(range(lo, rng.randint(lo, n - 1) + 1))
    else:
        owned = {l for l in range(n) if rng.random() < rng.choice([0.3, 0.7, 1.0])}
    if rng.random() < 0.2:
        bounds = None
    else:
        if rng.random() < 0.5:                       # a uniform index set: the last region takes the remainder
            sizes = [3] * (n - 1) + [rng.choice([3, 4, 0])]
        else:
            sizes = [rng.choice([0, 3, 3, 3, 5]) for _ in range(n)]
        starts = [sum(sizes[:l]) for l in range(n)]
        bounds = [(starts[l], starts[l] + sizes[l]) for l in range(n)]
    weight = rng.choice([0, 1, 7, 100])
    budget = rng.choice([0, 1, 20, 350, 1000, 0.5 * 701, 10 ** 9])
    return regions, owned, bounds, (lambda ns: weight * (ns or 1)), budget


def test_plan_properties_on_random_inputs():
    rng = random.Random(20240229)
    batched_some = 0
    for _ in range(400):
        regions, owned, bounds, per_block, budget = _random_case(rng)
        calls, covered = plan_batched_calls(regions, owned, bounds, per_block, budget)
        taken = []
        for i0, nb, ns, rows in calls:
            assert nb >= 1 and 0 <= i0 and i0 + nb <= len(regions)               # a contiguous arena run ...
            members = regions[i0:i0 + nb]
            assert all(l in owned for l in members)
            if bounds is None:
                assert ns is None and rows == []
            else:
                assert ns > 0                                                     # ... of equal ns > 0 ...
                assert all(bounds[l][1] - bounds[l][0] == ns for l in members)
                assert rows == [bounds[l][0] for l in members]
            assert nb <= max(1, budget // max(1, per_block(ns)))                  # ... within the budget
            taken.extend(members)
        assert len(taken) == len(set(taken))                                      # sub-batches are disjoint
        assert set(taken) == covered                                              # and their union is what is covered
        rest = owned - covered
        assert covered <= owned and covered | rest == owned and not covered & rest
        assert (sorted(calls, key=lambda c: c[0]), covered) == _expected(regions, owned, bounds, per_block, budget)
        batched_some += bool(calls)
    assert batched_some > 100                                                     # a quarter of the cases at least are batched
