"""The slot schedule of LlmEngine.generate_continuous as a pure function (no GPU): plan_slots on hand-checked inputs, and its
bound against the schedule without slots (arrival-order groups, each run to its longest request)."""
from fangyan_tts_amd import synth
from fangyan_tts_amd.llm import grouped_steps, plan_slots


def issue_bound(lens, n_slots, poll):
    """sum over arrival-order groups of n_slots of the group's longest length, rounded up to the poll"""
    return sum(-(-max(lens[g: g + n_slots]) // poll) * poll for g in range(0, len(lens), n_slots))


def test_fewer_requests_than_slots_is_one_group():
    steps, joins = plan_slots([5, 9, 3], 4, 8)
    assert joins == [(0, [(0, 0), (1, 1), (2, 2)])]          # request r into slot r, before any step
    assert steps == 8                                        # the longest needs 9 - 1 = 8 steps after its join: one poll
    assert plan_slots([5, 10, 3], 4, 8)[0] == 16             # 9 steps: two polls
    assert plan_slots([1], 4, 8)[0] == 8                     # the join emits the only token; one poll sees it ended
    assert plan_slots([], 4, 8) == (0, [])


def test_lowest_free_slot_in_arrival_order():
    steps, joins = plan_slots([20, 3, 3, 3, 30, 4], 2, 8)
    # t = 0: r0 -> slot 0 (19 steps), r1 -> slot 1 (2).  t = 8: slot 1 free -> r2.  t = 16: r3.  t = 24: slots 0 and 1 free -> r4, r5.
    # r4 needs 29 steps: four polls, 24 + 32 = 56
    assert joins == [(0, [(0, 0), (1, 1)]), (8, [(2, 1)]), (16, [(3, 1)]), (24, [(4, 0), (5, 1)])]
    assert steps == 56
    assert grouped_steps([20, 3, 3, 3, 30, 4], 2, 8) == 24 + 8 + 32


def test_one_long_sequence_per_group():
    """Every group of 4 has one request of 81 tokens (80 steps) beside three of 9 (8 steps): grouped, each group costs 80 steps;
    with slots the short ones pass through three slots while the long ones hold one each until all four slots hold a long one."""
    lens = [81, 9, 9, 9] * 4
    assert grouped_steps(lens, 4, 8) == 4 * 80
    steps, joins = plan_slots(lens, 4, 8)
    # t=0: L0 s0, three short.  t=8: r4 = L1 -> s1, r5, r6 -> s2, s3.  t=16: r7 -> s2, L2 -> s3.  t=24: r9 -> s2.  t=32: r10.  t=40: r11.
    # t=48: L3 -> s2, ends at 128.  All four slots hold a long one: r13 waits for slot 0 (free at 80); at 88 slot 0 is free again
    # and slot 1 (joined at 8) too: r14, r15
    assert [t for t, _ in joins] == [0, 8, 16, 24, 32, 40, 48, 80, 88]
    assert joins[6][1] == [(12, 2)] and joins[7][1] == [(13, 0)] and joins[8][1] == [(14, 0), (15, 1)]
    assert steps == 128


def test_never_more_steps_than_the_grouped_schedule():
    for k in range(300):
        n = int(synth.randint(f"slots.cpu.n.{k}", (1,), 1, 70)[0])
        n_slots = int(synth.randint(f"slots.cpu.s.{k}", (1,), 1, 13)[0])
        poll = int(synth.randint(f"slots.cpu.p.{k}", (1,), 1, 17)[0])
        lens = synth.randint(f"slots.cpu.len.{k}", (n,), 1, 251).tolist()
        steps, joins = plan_slots(lens, n_slots, poll)
        assert steps <= grouped_steps(lens, n_slots, poll) <= issue_bound(lens, n_slots, poll) + poll * (-(-n // n_slots)), (k, lens, n_slots, poll)
        assert steps % poll == 0
        joined = [r for _, batch in joins for r, _ in batch]
        assert joined == list(range(n))                      # everyone joins, in arrival order
        assert all(0 <= s < n_slots for _, batch in joins for _, s in batch)
        if n <= n_slots:
            assert steps == grouped_steps(lens, n_slots, poll) and len(joins) == 1
