"""`plan_serve_stream` (fangyan_tts_amd/flow.py): the streaming serving loop's schedule as a pure function - stream=True requests
join slots as they fall free, every stream gets at most one chunk per poll.  No GPU, no library."""
import random

import pytest

from fangyan_tts_amd.flow import plan_serve_stream, stream_chunk_plan, stream_poll_plan


def random_case(rng, n_max=12):
    N = rng.randint(1, n_max)
    n_tokens = [rng.randint(1, 260) for _ in range(N)]
    prompts = [rng.choice([0, 7, 12, 25, 30, 49, 50, 51]) for _ in range(N)]
    arrivals, a = [], 0
    for _ in range(N):
        a += rng.choice([0, 0, 1, 2, 5])
        arrivals.append(a)
    return n_tokens, prompts, arrivals, rng.randint(1, 5), rng.choice([25, 25, 8, 40])


def grouped_polls(n_tokens, prompts, n_slots, tpp=25):
    """Polls the parent's way takes: arrival-order groups of n_slots, each through `stream_poll_plan` to its end."""
    return sum(len(stream_poll_plan(n_tokens[g: g + n_slots], prompts[g: g + n_slots], tpp)) for g in range(0, len(n_tokens), n_slots))


def test_every_request_gets_its_own_chunk_plan_in_order():
    rng = random.Random(1986)
    for _ in range(300):
        n_tokens, prompts, arrivals, n_slots, tpp = random_case(rng)
        polls = plan_serve_stream(n_tokens, prompts, arrivals, n_slots, tpp)
        for r in range(len(n_tokens)):
            mine = [c[1:] for p in polls for c in p["chunks"] if c[0] == r]
            assert mine == stream_chunk_plan(n_tokens[r], prompts[r]), (r, n_tokens, prompts, arrivals, n_slots, tpp)
        for p in polls:                                       # at most one chunk per stream and poll
            assert len({c[0] for c in p["chunks"]}) == len(p["chunks"])
        # a request never joins before it arrives, and its first chunk never comes before its join
        joined = {r: k for k, p in enumerate(polls) for r, _ in p["joins"]}
        assert sorted(joined) == list(range(len(n_tokens)))
        assert all(joined[r] >= arrivals[r] for r in joined)
        first = {}
        for k, p in enumerate(polls):
            for c in p["chunks"]:
                first.setdefault(c[0], k)
        assert all(first[r] >= joined[r] for r in joined)


def test_all_present_and_no_more_than_slots_is_stream_poll_plan():
    rng = random.Random(7)
    for _ in range(300):
        n_tokens, prompts, _, _, tpp = random_case(rng, 6)
        n_slots = len(n_tokens) + rng.randint(0, 2)
        polls = plan_serve_stream(n_tokens, prompts, None, n_slots, tpp)
        assert [p["chunks"] for p in polls] == stream_poll_plan(n_tokens, prompts, tpp), (n_tokens, prompts, tpp)
        assert polls[0]["joins"] == [(r, r) for r in range(len(n_tokens))] and not any(p["joins"] for p in polls[1:])


def test_slots_are_held_once_and_refilled_lowest_first_in_arrival_order():
    rng = random.Random(42)
    for _ in range(300):
        n_tokens, prompts, arrivals, n_slots, tpp = random_case(rng)
        polls = plan_serve_stream(n_tokens, prompts, arrivals, n_slots, tpp)
        held, waiting, nxt, order = {}, [], 0, []
        for k, p in enumerate(polls):
            while nxt < len(n_tokens) and arrivals[nxt] <= k:
                waiting.append(nxt)
                nxt += 1
            free = [s for s in range(n_slots) if s not in held]             # (what fell free in this poll is not among them yet)
            want = list(zip(waiting, free))                                   # arrival order into the lowest free slots
            assert p["joins"] == want, (k, n_tokens, prompts, arrivals, n_slots)
            for r, s in p["joins"]:
                assert s not in held                                          # no slot is held twice
                held[s] = r
                waiting.remove(r)
                order.append(r)
            finals = sorted(s for s in held if any(c[0] == held[s] and c[3] for c in p["chunks"]))
            assert p["released"] == finals                                    # the final pass releases the slot, in its poll
            for c in p["chunks"]:
                assert c[0] in held.values()
            for s in p["released"]:
                del held[s]                                                   # ... and it can be joined from the next poll on
        assert order == list(range(len(n_tokens))) and not held and not waiting


# (n_tokens, prompts, n_slots) -> (polls of the loop, polls of arrival-order groups through stream_poll_plan), worked out from the
# rules: 25 tokens per poll from the join; the first chunk needs 25 + pad + 3 tokens, each further one 25 more; a stream has its
# final pass in the first poll in which all its tokens are there and no further chunk is complete.  Alone: 20 tokens take 1 poll,
# 30 take 3 (-, chunk 28, final), 60 take 4, 100 take 5, 120 take 6, 200 take 9.
FIXED = [
    # one slot: 4 + 1 + 6 polls back to back either way (a slot released in a poll is joined in the next)
    (([60, 20, 120], [0, 0, 0], 1), (11, 11)),
    # two slots: groups (100, 30) and (30, 100) need 5 + 5; the loop joins request 2 in poll 3 and request 3 in poll 5, which then
    # needs its own 5 polls: nothing gained, nothing lost
    (([100, 30, 30, 100], [0, 0, 0, 0], 2), (10, 10)),
    # two slots: groups (200, 20), (20, 20), (20,) need 9 + 1 + 1; the loop serves the short ones beside the long one
    (([200, 20, 20, 20, 20], [0, 0, 0, 0, 0], 2), (9, 11)),
    # three slots, prompts that pad the first hop (12 -> 13 more tokens, 30 -> 20 more): groups (130, 40, 55) and (90, 26) need 6 + 4
    (([130, 40, 55, 90, 26], [12, 30, 0, 12, 25], 3), (6, 10)),
]


@pytest.mark.parametrize("case,want", FIXED)
def test_no_more_polls_than_arrival_order_groups(case, want):
    n_tokens, prompts, n_slots = case
    polls = plan_serve_stream(n_tokens, prompts, None, n_slots)
    assert (len(polls), grouped_polls(n_tokens, prompts, n_slots)) == want
    assert len(polls) <= grouped_polls(n_tokens, prompts, n_slots)


def test_never_more_polls_than_groups_when_all_are_present():
    rng = random.Random(3)
    for _ in range(300):
        n_tokens, prompts, _, n_slots, tpp = random_case(rng)
        assert len(plan_serve_stream(n_tokens, prompts, None, n_slots, tpp)) <= grouped_polls(n_tokens, prompts, n_slots, tpp)


def test_idle_polls_between_arrivals_and_bad_input():
    polls = plan_serve_stream([20, 20], [0, 0], [0, 4], 2)
    assert [bool(p["joins"]) for p in polls] == [True, False, False, False, True]
    assert polls[1] == {"joins": [], "chunks": [], "released": []}
    assert polls[4] == {"joins": [(1, 0)], "chunks": [(1, 20, 0, True)], "released": [0]}
    with pytest.raises(AssertionError):
        plan_serve_stream([4, 4], [0, 0], [3, 1], 2)          # arrival polls out of request order
    with pytest.raises(AssertionError):
        plan_serve_stream([4, 0], [0, 0], None, 2)
