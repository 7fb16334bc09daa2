"""`plan_serve` (fangyan_tts_amd/llm.py): the serving loop's schedule as a pure function - joins into the LM's decode slots,
retirements, flow groups.  Properties on hand-made cases and on seeded random ones; no GPU."""
import random

import pytest

from fangyan_tts_amd.llm import plan_serve, plan_slots


def check_plan(n_tokens, arrivals, n_slots, spp, gmax, gwait):
    """Every structural property of a plan; returns (polls, joined_at, retired_at, grouped_at, groups in order)."""
    N = len(n_tokens)
    arr = [0] * N if arrivals is None else list(arrivals)
    polls = plan_serve(n_tokens, arrivals, n_slots, spp, gmax, gwait)
    assert [p["poll"] for p in polls] == list(range(len(polls)))
    joined_at, slot_of, retired_at, grouped_at, order = {}, {}, {}, {}, []
    occupied = {}                                            # slot -> request, replayed
    ready = []                                               # retired and not yet grouped, oldest first
    next_join = 0
    for p in polls:
        k = p["poll"]
        free = sorted(s for s in range(n_slots) if s not in occupied)
        waiting = [r for r in range(next_join, N) if arr[r] <= k]
        # one join: the requests that have arrived, in arrival order, into the lowest free slots - as many as fit
        assert p["joins"] == list(zip(waiting, free)), (k, p["joins"], waiting, free)
        for r, s in p["joins"]:
            assert r not in joined_at and s not in occupied and 0 <= s < n_slots
            joined_at[r], slot_of[r] = k, s
            occupied[s] = r
        next_join += len(p["joins"])
        assert p["steps"] == (spp if occupied else 0)
        assert [s for _, s in p["retired"]] == sorted(s for _, s in p["retired"])
        for r, s in p["retired"]:
            assert occupied.get(s) == r and r not in retired_at
            # the join emits the first token: n - 1 token steps, seen ended in the first poll that has run that many
            assert k - joined_at[r] + 1 == max(1, -(-(n_tokens[r] - 1) // spp)), (r, k)
            retired_at[r] = k
            del occupied[s]
            ready.append(r)
        for g in p["groups"]:
            assert 1 <= len(g) <= gmax
            assert sorted(g, key=ready.index) == ready[: len(g)], "groups are cut oldest first"
            assert [n_tokens[r] for r in g] == sorted((n_tokens[r] for r in g), reverse=True), "longest first inside a group"
            for a, b in zip(g, g[1:]):
                assert n_tokens[a] > n_tokens[b] or ready.index(a) < ready.index(b), "equal lengths keep their retirement order"
            for r in g:
                assert r not in grouped_at
                grouped_at[r] = k
            ready = ready[len(g):]
            order.append(g)
        # after the cut: fewer than group_max wait, none of them for group_wait polls or more, none once all else is done
        assert len(ready) < gmax
        assert all(k - retired_at[r] < gwait for r in ready), (k, ready)
        if not occupied and next_join == N:
            assert not ready
    assert sorted(joined_at) == sorted(retired_at) == sorted(grouped_at) == list(range(N))
    assert all(grouped_at[r] - retired_at[r] <= gwait for r in range(N))
    assert not occupied and not ready
    return polls, joined_at, retired_at, grouped_at, order


def test_by_hand_two_slots():
    """Lengths 9 / 17 / 5 / 9 through 2 slots, 8 steps per poll, groups of 2, wait 1:
    poll 0: r0 -> slot 0, r1 -> slot 1; r0 (8 steps) ends.  poll 1: r2 -> slot 0; r1 (16) and r2 (4) end: with r0 three are ready,
    the two oldest go (r1 the longer first), r2 stays.  poll 2: r3 -> slot 0 ends; with r2 that is a full group."""
    polls = plan_serve([9, 17, 5, 9], None, 2, 8, 2, 1)
    assert polls == [
        {"poll": 0, "joins": [(0, 0), (1, 1)], "steps": 8, "retired": [(0, 0)], "groups": []},
        {"poll": 1, "joins": [(2, 0)], "steps": 8, "retired": [(2, 0), (1, 1)], "groups": [(0, 2)]},
        {"poll": 2, "joins": [(3, 0)], "steps": 8, "retired": [(3, 0)], "groups": [(1, 3)]},
    ]


def test_by_hand_wait_and_drain():
    """One slot, groups of up to 3, wait 2: r0 retires in poll 0 and waits polls 1 and 2 at the most - it leaves in poll 2 with r1
    (retired in poll 1) and r2 (poll 2: a full group); r3 retires in poll 3 with nothing left under way and leaves alone, at once."""
    polls = plan_serve([4, 6, 5, 3], None, 1, 8, 3, 2)
    assert [p["groups"] for p in polls] == [[], [], [(1, 2, 0)], [(3,)]]
    polls = plan_serve([4, 6, 5, 3], None, 1, 8, 3, 1)
    assert [p["groups"] for p in polls] == [[], [(1, 0)], [], [(2, 3)]]
    polls = plan_serve([4, 6, 5, 3], None, 1, 8, 3, 0)
    assert [p["groups"] for p in polls] == [[(0,)], [(1,)], [(2,)], [(3,)]]


def test_by_hand_arrivals():
    """Two requests at poll 0, three more at poll 4 (3 slots): the slots idle in polls 2 and 3 (no steps), the late ones join
    together in poll 4 into slots 0, 1, 2."""
    polls = plan_serve([12, 9, 5, 20, 5], [0, 0, 4, 4, 4], 3, 8, 3, 2)
    assert [p["joins"] for p in polls] == [[(0, 0), (1, 1)], [], [], [], [(2, 0), (3, 1), (4, 2)], [], []]
    assert [p["steps"] for p in polls] == [8, 8, 0, 0, 8, 8, 8]
    assert [p["retired"] for p in polls] == [[(1, 1)], [(0, 0)], [], [], [(2, 0), (4, 2)], [], [(3, 1)]]
    # r1 waits two polls (0 -> 2) and leaves with r0; r2 and r4 wait for r3 two polls and leave with it as it retires
    assert [p["groups"] for p in polls] == [[], [], [(0, 1)], [], [], [], [(3, 2, 4)]]


def test_lengths_sort_the_groups_not_the_schedule():
    """lengths (the counts after the silent-token filter) order a group; the retirement polls follow n_tokens alone."""
    a = plan_serve([9, 9, 9], None, 3, 8, 3, 0)
    b = plan_serve([9, 9, 9], None, 3, 8, 3, 0, lengths=[4, 9, 6])
    assert [p["retired"] for p in a] == [p["retired"] for p in b]
    assert a[0]["groups"] == [(0, 1, 2)] and b[0]["groups"] == [(1, 2, 0)]


def rand_case(seed):
    rng = random.Random(seed)
    N = rng.randint(1, 40)
    n_tokens = [rng.randint(1, 60) for _ in range(N)]
    n_slots, spp = rng.randint(1, 9), rng.choice([1, 3, 8, 8, 16])
    gmax, gwait = rng.randint(1, 6), rng.randint(0, 4)
    if rng.random() < 0.4:
        arrivals = None
    else:
        arrivals = sorted(rng.randint(0, 12) for _ in range(N))
    return n_tokens, arrivals, n_slots, spp, gmax, gwait


@pytest.mark.parametrize("block", range(6))
def test_random_plans(block):
    for seed in range(50 * block, 50 * block + 50):
        n_tokens, arrivals, n_slots, spp, gmax, gwait = rand_case(seed)
        check_plan(n_tokens, arrivals, n_slots, spp, gmax, gwait)


def test_group_max_one_gives_singletons_in_retirement_order():
    for seed in range(100):
        n_tokens, arrivals, n_slots, spp, _, gwait = rand_case(seed)
        polls, *_ = check_plan(n_tokens, arrivals, n_slots, spp, 1, gwait)
        retired = [r for p in polls for r, _ in p["retired"]]
        groups = [g for p in polls for g in p["groups"]]
        assert groups == [(r,) for r in retired]
        for p in polls:                                      # ... and each in the poll it retires in
            assert p["groups"] == [(r,) for r, _ in p["retired"]]


def test_token_steps_equal_plan_slots():
    for seed in range(200):
        n_tokens, _, n_slots, spp, gmax, gwait = rand_case(seed)
        polls = plan_serve(n_tokens, None, n_slots, spp, gmax, gwait)
        steps, joins = plan_slots(n_tokens, n_slots, spp)
        assert sum(p["steps"] for p in polls) == steps, seed
        got, t = [], 0
        for p in polls:
            if p["joins"]:
                got.append((t, p["joins"]))
            t += p["steps"]
        assert got == joins, seed
    # README "Decode slots": 128 ragged requests through 32 slots
    assert sum(p["steps"] for p in plan_serve([5 + (37 * i) % 90 for i in range(128)], None, 32, 8, 8, 2)) == plan_slots(
        [5 + (37 * i) % 90 for i in range(128)], 32, 8)[0]


def test_bad_arguments():
    with pytest.raises(AssertionError):
        plan_serve([4, 4], [3, 1], 2, 8, 2, 2)               # arrival polls out of request order
    with pytest.raises(AssertionError):
        plan_serve([4, 0], None, 2, 8, 2, 2)
    with pytest.raises(AssertionError):
        plan_serve([4], None, 2, 8, 0, 2)
