"""The schedules of tests/test_seq_ring_gpu.py run through the restatement of the ring bookkeeping (tests/seq_ring_reference.py): the
properties that make the GPU scenarios meaningful -- they wrap several times, skip tails, leave never-written rows behind, repeat their rows
from the second lap on, are legal throughout, and stop being legal exactly where the rule says. CPU only."""
import pytest

from tests import seq_ring_reference as rr

LP = {"gato": 37, "gpt": 7}   # the prompt length of the GPU tests' layout (below); the properties hold for any Lp


def test_prompt_lengths_of_the_gpu_scenario():
    from oracle.cases import BASELINE_CASES
    from vima_amd.policy import build_prompt_index
    layout = BASELINE_CASES["baseline_gato"]["layout"]
    assert {k: build_prompt_index(layout, rr.Q[k])[1] for k in LP} == LP


@pytest.mark.parametrize("kind,wraps,tails", [("gato", 5, [6, 5, 5, 5, 5]), ("gpt", 6, [0, 1, 1, 1, 1, 1])])
def test_scenario_is_legal_wraps_and_skips_tails(kind, wraps, tails):
    ring, log = rr.run_schedule(kind, LP[kind])          # no Refused: every one of the 26 steps is legal
    assert len(log) == rr.STEPS
    wrapped = [s for s in log if s["wrap"]]
    assert len(wrapped) == wraps and [s["tail"] for s in wrapped] == tails
    assert all(s["row"] == ring.P0 for s in wrapped)
    assert all(s["tail"] == 0 for s in log if not s["wrap"])
    assert all(ring.P0 <= s["row"] and s["row"] + s["Lq"] <= s["hw"] <= ring.Lmax for s in log)
    assert log[0]["Lq"] == rr.Q[kind] and all(s["Lq"] == rr.Q[kind] + 1 for s in log[1:])
    assert max(rr.lap_of_step(log)) == wraps + 1


def test_gato_leaves_rows_that_are_never_written():
    ring, log = rr.run_schedule("gato", LP["gato"])
    assert ring.hw == ring.P0 + 85 < ring.Lmax            # rows [P0 + 85, Lmax) exist and must never be read
    written = set()
    for s in log:
        assert s["hw"] <= ring.P0 + 85
        assert all(r in written or s["row"] <= r < s["row"] + s["Lq"] for r in range(ring.P0, s["hw"])), "the step would read an unwritten row"
        written.update(range(s["row"], s["row"] + s["Lq"]))
    assert written == set(range(ring.P0, ring.P0 + 85))
    # the first lap is one row shorter (step 0 has no action slot): hw moves once more at the end of the second lap
    assert [s["hw"] - ring.P0 for s in log[:11]] == [16, 33, 50, 67, 84, 84, 84, 84, 84, 85, 85]


def test_gpt_reaches_the_last_row():
    ring, log = rr.run_schedule("gpt", LP["gpt"])
    assert ring.hw == ring.Lmax                           # the first lap (1 + 4 * 2 rows) fills the ring exactly: its wrap skips nothing
    assert ring.Lmax < 64 < LP["gato"] + 1 + 85           # the two sides of the attention launcher's choice by key count


@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_laps_repeat_from_the_second_on(kind):
    ring, log = rr.run_schedule(kind, LP[kind])
    laps = rr.lap_of_step(log)
    rows = {}
    for lap, s in zip(laps, log):
        rows.setdefault(lap, []).append((s["row"], s["Lq"]))
    full = [lap for lap in rows if 2 <= lap < max(rows)]   # the last lap of the schedule is cut short
    assert len(full) >= 3
    assert all(rows[lap] == rows[2] for lap in full) and rows[2][0][0] == ring.P0
    assert rows[max(rows)] == rows[2][:len(rows[max(rows)])]
    assert rows[1] != rows[2]                              # step 0 has Q rows: the first lap is its own
    # what a captured graph bakes in: (row, hw, action slot). hw stops moving at the end of lap 2 (gato) / lap 1 (gpt), so the set of keys is
    # complete one lap later and stays as it is
    keys = rr.graph_keys(log)
    first_of_lap = {lap: laps.index(lap) for lap in set(laps)}
    done = 4 if kind == "gato" else 3
    assert set(keys[:first_of_lap[done]]) == set(keys)
    assert len(set(keys[:first_of_lap[done - 1]])) < len(set(keys))


@pytest.mark.parametrize("kind,ages,advance", [("gato", [17, 34, 84], 23), ("gpt", [2, 4, 9], 2)])
def test_a_sample_that_is_never_restarted_is_refused_at_step_5(kind, ages, advance):
    with pytest.raises(rr.Refused) as ei:
        rr.run_schedule(kind, LP[kind], never=(2,))
    e = ei.value
    assert (e.step, e.sample, e.age, e.advance) == (5, 2, ages[2], advance)
    assert e.ring.age == ages and len(e.log) == 5          # nothing changed: the ring is as the fifth successful step left it
    assert e.ring.steps_left()[2] == 0 and min(e.ring.steps_left()[:2]) > 0
    e.ring.restart([False, False, True])
    assert e.ring.steps_left()[2] > 0
    e.ring.step()


def test_the_legality_rule_is_sharp():
    """One row fewer per lap than five whole steps need (R = 73 = 16 + 3 * 17 + 6): the schedule that R = 90 carries is refused at step 7."""
    with pytest.raises(rr.Refused) as ei:
        rr.run_schedule("gato", LP["gato"], R=73)
    assert ei.value.step == 7
    rr.run_schedule("gato", LP["gato"], R=90)


@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_steps_left_is_the_bookkeeping_run_forward(kind):
    """steps_left()[b] == n means: with sample b never restarted again (everybody else restarted at will), exactly n more steps succeed."""
    ring, _ = rr.run_schedule(kind, LP[kind], steps=7)
    for b in range(rr.B):
        left = ring.steps_left()[b]
        sim = rr.Ring(LP[kind], ring.Lmax, rr.Q[kind], rr.B)
        sim.wp, sim.hw, sim.age, sim.next = ring.wp, ring.hw, list(ring.age), ring.next
        n = 0
        while True:
            sim.restart([bb != b for bb in range(rr.B)])
            try:
                sim.step()
            except rr.Refused as e:
                assert e.sample == b
                break
            n += 1
        assert n == left
    # before step 0 the first step has Q rows
    fresh = rr.Ring(LP[kind], ring.Lmax, rr.Q[kind], rr.B)
    want = 1 + (rr.RING[kind] - rr.Q[kind]) // (rr.Q[kind] + 1)
    assert fresh.steps_left() == [want] * rr.B


def test_linear_formula():
    assert rr.linear_steps_left(64, 19, 16, True) == 2 and rr.linear_steps_left(64, 35, 16, False) == 1 and rr.linear_steps_left(64, 52, 16, False) == 0
