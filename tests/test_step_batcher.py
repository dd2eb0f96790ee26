"""CPU tests of the step-level scheduler (batcher.StepBatcher) with an injected step: the pure parts (grid, admission plan, slot
book, solver rotation) and the loop's contract -- who shares an iteration, how many steps each request gets and at which times,
slot recycling, error release, close()."""
import threading
import time

import pytest
import torch

from conftest import sub


@pytest.fixture(scope="module")
def bt():
    return sub("batcher")


def test_step_grid_is_the_fp32_linspace_of_cfm_forward(bt):
    for n in (1, 2, 3, 4, 7, 10, 32):
        span = torch.linspace(0, 1, n + 1, dtype=torch.float32)
        grid = bt.step_grid(n)
        assert len(grid) == n
        for i, (t0, t1) in enumerate(grid):
            assert t0 == float(span[i]) and t1 == float(span[i + 1])
            assert abs(t0 - i / n) < 1.2e-7                      # i / n to fp32 rounding (linspace's own arithmetic decides the last bit)
            # dt as the device takes it: the fp32 difference of fp32 neighbours
            assert float(torch.tensor(t1, dtype=torch.float32) - torch.tensor(t0, dtype=torch.float32)) == float(span[i + 1] - span[i])
        assert grid[0][0] == 0.0 and grid[-1][1] == 1.0
    with pytest.raises(ValueError):
        bt.step_grid(0)


def test_admission_plan(bt):
    R = lambda n: bt.Request(ids=[1] * n)
    w = [R(10), R(20), R(5), R(40)]
    assert bt.plan_admission(w, 0, 0, 8, 8, 1000) == [0, 1, 2, 3]
    assert bt.plan_admission(w, 0, 0, 2, 8, 1000) == [0, 1]                      # two free slots
    assert bt.plan_admission(w, 6, 30, 8, 8, 1000) == [0, 1]                     # max_batch - active = 2
    assert bt.plan_admission(w, 8, 30, 8, 8, 1000) == []
    assert bt.plan_admission(w, 0, 0, 0, 8, 1000) == []
    # budget = requests x longest: 10 | 20 -> 40; +5 -> 60; +40 would be 160 > 100: skipped, not waited for
    assert bt.plan_admission(w, 0, 0, 8, 8, 100) == [0, 1, 2]
    assert bt.plan_admission([R(40), R(5)], 2, 30, 8, 8, 100) == [1]             # 3 x 40 > 100, 3 x 30 fits
    assert bt.plan_admission([R(500)], 0, 0, 8, 8, 100) == [0]                   # nothing active: the head goes alone
    assert bt.plan_admission([], 0, 0, 8, 8, 100) == []


def test_slot_book_and_solver_rotation(bt):
    s = bt.SlotBook(3)
    assert [s.take(), s.take(), s.take()] == [0, 1, 2] and s.n_free == 0
    with pytest.raises(RuntimeError):
        s.take()
    s.release(1)
    with pytest.raises(RuntimeError):
        s.release(1)
    assert s.take() == 1
    s.release(2), s.release(0)
    assert s.take() == 0                                                         # lowest free index first
    assert bt.next_solver([], None) is None
    assert bt.next_solver(["midpoint", "euler", "euler"], None) == "euler"
    assert bt.next_solver(["midpoint", "euler"], "euler") == "midpoint"
    assert bt.next_solver(["midpoint", "euler"], "midpoint") == "euler"
    assert bt.next_solver(["euler"], "rk4") == "euler"


class Recorder:
    """A fake device step: logs (solver, [(request tag, slot, step index, t0, t1)]) per iteration."""

    def __init__(self, seconds=0.0, fail_at=None):
        self.log, self.seconds, self.fail_at = [], seconds, fail_at
        self.first = threading.Event()

    def __call__(self, solver, entries):
        self.log.append((solver, [(e.request.ids[0], e.slot, e.i, e.t0, e.t1) for e in entries]))
        self.first.set()
        if self.fail_at is not None and len(self.log) == self.fail_at:
            raise RuntimeError("device on fire")
        time.sleep(self.seconds)

    def steps_of(self, tag):
        return [(i, t0, t1) for _, es in self.log for (g, _, i, t0, t1) in es if g == tag]


def test_a_request_joins_a_running_solve_at_the_next_iteration(bt):
    run = Recorder(seconds=0.02)
    with bt.StepBatcher(None, max_batch=4, run_step=run) as q:
        a = q.submit([1] * 6, solver="euler", n_timesteps=6)
        assert run.first.wait(5)                                    # a is mid-solve
        b = q.submit([2] * 3, solver="euler", n_timesteps=2)
        ra, rb = a.result(5), b.result(5)
    assert ra["mel_length"] == 6 and rb["mel_length"] == 3
    first_b = next(k for k, (_, es) in enumerate(run.log) if any(g == 2 for g, *_ in es))
    assert 1 <= first_b <= 2                                        # not after a's solve (6 iterations): at the next iteration
    assert any({g for g, *_ in es} == {1, 2} for _, es in run.log)  # they shared iterations
    assert len(run.log) == 6                                        # b's two steps cost no iteration of their own
    # each request got exactly its steps, in order, at its own grid's times
    for tag, n in ((1, 6), (2, 2)):
        grid = bt.step_grid(n)
        assert run.steps_of(tag) == [(i, grid[i][0], grid[i][1]) for i in range(n)]
    assert q.utterance_steps == 8 and q.batches_run == 6


def test_mixed_step_counts_share_iterations_and_solvers_never_do(bt):
    run = Recorder(seconds=0.005)
    with bt.StepBatcher(None, max_batch=8, run_step=run) as q:
        futs = [q.submit([10 + k] * 4, solver=s, n_timesteps=n) for k, (s, n) in
                enumerate([("euler", 2), ("euler", 4), ("midpoint", 10), ("euler", 10), ("midpoint", 3), ("rk4", 1)])]
        for f in futs:
            f.result(10)
    spec = {10: ("euler", 2), 11: ("euler", 4), 12: ("midpoint", 10), 13: ("euler", 10), 14: ("midpoint", 3), 15: ("rk4", 1)}
    for solver, es in run.log:
        assert es and all(spec[g][0] == solver for g, *_ in es)     # one solver per iteration
        assert len({slot for _, slot, *_ in es}) == len(es)         # distinct slots
    for tag, (solver, n) in spec.items():
        grid = bt.step_grid(n)
        assert run.steps_of(tag) == [(i, grid[i][0], grid[i][1]) for i in range(n)]
    assert any(len({spec[g][1] for g, *_ in es}) > 1 for _, es in run.log)       # different n_timesteps in one iteration
    assert {s for s, _ in run.log} == {"euler", "midpoint", "rk4"}


def test_slots_are_recycled_and_bound_the_active_set(bt):
    run = Recorder()
    with bt.StepBatcher(None, max_batch=8, n_slots=2, run_step=run) as q:
        futs = [q.submit([k + 1] * 2, solver="euler", n_timesteps=2) for k in range(7)]
        for f in futs:
            f.result(10)
    assert {slot for _, es in run.log for _, slot, *_ in es} == {0, 1}
    assert max(len(es) for _, es in run.log) <= 2
    assert sorted({g for _, es in run.log for g, *_ in es}) == list(range(1, 8))
    assert q.slots.n_free == 2


def test_an_exception_in_a_step_releases_every_future_and_the_batcher_goes_on(bt):
    run = Recorder(seconds=0.01, fail_at=2)
    with bt.StepBatcher(None, max_batch=4, run_step=run) as q:
        a = q.submit([1] * 3, solver="euler", n_timesteps=5)
        b = q.submit([2] * 3, solver="euler", n_timesteps=5)
        for f in (a, b):
            with pytest.raises(RuntimeError, match="on fire"):
                f.result(5)
        assert q.slots.n_free == q.slots.n_slots
        c = q.submit([3] * 3, solver="euler", n_timesteps=2)        # the worker is still alive
        assert c.result(5)["mel_length"] == 3


def test_close_completes_the_work_in_flight_and_refuses_new_work(bt):
    run = Recorder(seconds=0.01)
    q = bt.StepBatcher(None, max_batch=2, run_step=run)
    futs = [q.submit([k + 1] * 2, solver="midpoint", n_timesteps=4) for k in range(5)]      # more than fit at once
    q.close()
    assert all(f.done() and f.result()["mel_length"] == 2 for f in futs)
    with pytest.raises(RuntimeError):
        q.submit([1, 2])
    with pytest.raises(ValueError):
        bt.StepBatcher(None, run_step=run).submit([])


def test_speech_service_takes_either_batcher(bt):
    serving = sub("serving")
    run = Recorder()
    with bt.StepBatcher(None, max_batch=4, run_step=run) as q:
        svc = serving.SpeechService(q, phonemize=lambda text, lang: [5] * len(text))
        res = svc.submit("hello", voice=0, speed=1.0, steps=3, solver="euler").result(5)
    assert res["mel_length"] == 5 and len(run.steps_of(5)) == 3
