"""`sampler._run_blocks`, the block loop of every device sampler, and `sampler._kept`, the slice rule of every
store, driven with plain Python callables: no GPU, no library."""
import threading

import pytest

from psfmc_amd.sampler import _kept, _run_blocks


class Recorder(object):
    """draw / launch callables that log (what, argument, thread) in call order."""

    def __init__(self):
        self.log = []

    def draw(self, n):
        self.log.append(('draw', n, threading.get_ident()))
        return 'draws%d' % len([e for e in self.log if e[0] == 'draw']), ['state'] * n

    def launch(self, draws):
        self.log.append(('launch', draws, threading.get_ident()))
        return 'result of ' + draws

    def calls(self, what):
        return [e[1] for e in self.log if e[0] == what]


@pytest.mark.parametrize('overlap', [True, False])
def test_block_sizes_and_order(overlap):
    rec = Recorder()
    out = list(_run_blocks(20, 7, rec.draw, rec.launch, overlap=overlap))
    assert rec.calls('draw') == [7, 7, 6]                     # and no fourth, never 0
    assert rec.calls('launch') == ['draws1', 'draws2', 'draws3']
    assert [(done, n, result) for done, n, result, _ in out] == [
        (0, 7, 'result of draws1'), (7, 7, 'result of draws2'), (14, 6, 'result of draws3')]
    assert [len(states) for _, _, _, states in out] == [7, 7, 6]


@pytest.mark.parametrize('overlap', [True, False])
def test_no_iterations_calls_nothing(overlap):
    rec = Recorder()
    assert list(_run_blocks(0, 7, rec.draw, rec.launch, overlap=overlap)) == []
    assert rec.log == []


def test_one_short_block_draws_once():
    rec = Recorder()
    out = list(_run_blocks(5, 64, rec.draw, rec.launch))
    assert rec.calls('draw') == [5] and rec.calls('launch') == ['draws1']
    assert [(done, n) for done, n, _, _ in out] == [(0, 5)]


def test_overlap_draws_the_next_block_during_the_launch():
    """Block k's launch does not return before the draw of block k + 1 has been entered: with the draw only after
    the launch this would wait out the time limit and fail."""
    log, entered = [], threading.Event()

    def draw(n):
        log.append(('draw', n))
        if len([e for e in log if e[0] == 'draw']) == 2:
            entered.set()
        return n, [None] * n

    def launch(draws):
        if draws == 7 and not [e for e in log if e[0] == 'launch']:
            assert entered.wait(30), 'the next draw was not entered while the launch ran'
        log.append(('launch', draws))
        return draws

    caller = threading.get_ident()
    threads = []
    blocks = _run_blocks(20, 7, draw, lambda d: (threads.append(threading.get_ident()), launch(d))[1])
    first = next(blocks)
    assert first[:3] == (0, 7, 7)
    assert log == [('draw', 7), ('draw', 7), ('launch', 7)]   # drawn ahead, before block 0 was yielded
    assert threads[0] != caller
    assert [b[:2] for b in blocks] == [(7, 7), (14, 6)]


def test_without_overlap_launch_runs_on_the_caller_and_the_draw_follows():
    rec = Recorder()
    blocks = _run_blocks(20, 7, rec.draw, rec.launch, overlap=False)
    next(blocks)
    assert [e[:2] for e in rec.log] == [('draw', 7), ('launch', 'draws1'), ('draw', 7)]
    list(blocks)
    assert [e[0] for e in rec.log] == ['draw', 'launch', 'draw', 'launch', 'draw', 'launch']
    assert {e[2] for e in rec.log} == {threading.get_ident()}


def test_a_failing_launch_raises_after_the_draw_beside_it():
    log = []

    def draw(n):
        log.append('draw in')
        log.append('draw out')
        return n, [None] * n

    def launch(draws):
        raise RuntimeError('launch failed')

    before = threading.active_count()
    with pytest.raises(RuntimeError, match='launch failed'):
        next(_run_blocks(20, 7, draw, launch))
    assert log == ['draw in', 'draw out'] * 2                 # the concurrent draw ran to its end first
    assert threading.active_count() == before


def test_a_failing_draw_still_joins_the_launch():
    release, finished = threading.Event(), []

    def draw(n):
        if release.is_set() or finished:
            raise AssertionError('drawn twice after the failure')
        if draw.calls:
            release.set()
            raise KeyError('draw failed')
        draw.calls += 1
        return n, [None] * n
    draw.calls = 0

    def launch(draws):
        assert release.wait(30)                               # still running when the draw fails
        finished.append(draws)
        return draws

    before = threading.active_count()
    with pytest.raises(KeyError, match='draw failed'):
        next(_run_blocks(20, 7, draw, launch))
    assert finished == [7]                                    # joined before the exception left the loop
    assert threading.active_count() == before


def test_kept_is_the_thinning_rule():
    """Iteration done + i of a block is kept iff (done + i) % thin == 0, at index (done + i) // thin."""
    cases = 0
    for done in range(13):
        for n in range(1, 10):
            for thin in range(1, 6):
                first, count, offset = _kept(done, n, thin)
                brute = [(i, (done + i) // thin) for i in range(n) if (done + i) % thin == 0]
                positions = list(range(n))[first::thin]
                assert len(positions) == count
                assert [(i, offset + j) for j, i in enumerate(positions)] == brute, (done, n, thin)
                cases += 1
    assert cases == 585
