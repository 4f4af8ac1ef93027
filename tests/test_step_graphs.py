"""step_graphs.StepGraphs, the eager / capture / replay state machine of every captured step, driven with fake captures:
no device, no library.  The fallback after a failed capture can only be checked here -- nobody makes a capture fail on a card."""
import pytest

from sketchyscenecolorization_amd import hip
from sketchyscenecolorization_amd.step_graphs import CAPTURED, EAGER, FAILED, REPLAYED, StepGraphs


class FakeGraph:
    def __init__(self, log=None):
        self.replays, self.log = 0, log

    def replay(self):
        self.replays += 1
        if self.log is not None:
            self.log.append(('replay',))


class Impl:
    calls = 0

    def __call__(self):
        self.calls += 1


def fake_capture(impl):
    impl()
    return FakeGraph()


def test_one_key_runs_eager_then_captures_then_replays():
    sg, impl = StepGraphs(), Impl()
    out, g = sg.run('k', impl, capture=fake_capture)
    assert (out, g) == (EAGER, None) and 'k' not in sg.graphs and impl.calls == 1
    out, g = sg.run('k', impl, capture=fake_capture)
    assert out == CAPTURED and sg.graphs['k'] is g and impl.calls == 2 and g.replays == 1
    for n in (2, 3):
        assert sg.run('k', impl, capture=fake_capture) == (REPLAYED, g)
        assert sg.graphs['k'] is g and g.replays == n
    assert impl.calls == 2


def test_keys_do_not_share_state():
    sg, a, b = StepGraphs(), Impl(), Impl()
    assert sg.run('a', a, capture=fake_capture)[0] == EAGER
    assert sg.run('a', a, capture=fake_capture)[0] == CAPTURED
    assert sg.run('b', b, capture=fake_capture)[0] == EAGER
    assert set(sg.graphs) == {'a'} and b.calls == 1
    assert sg.run('b', b, capture=fake_capture)[0] == CAPTURED
    assert sg.graphs['a'] is not sg.graphs['b'] and (a.calls, b.calls) == (2, 2)
    assert sg.graphs['a'].replays == 1 and sg.graphs['b'].replays == 1


def test_every_replay_is_stale_then_replay_then_one_refresh_per_flat(monkeypatch):
    log = []
    gen = [7]
    monkeypatch.setattr(hip, 'resplit_stale', lambda: log.append(('stale',)))
    monkeypatch.setattr(hip, 'refresh_new_splits', lambda flat, since: log.append(('refresh', flat, since)))
    monkeypatch.setattr(hip, 'split_generation', lambda: gen[0])

    def capture(impl):
        impl()
        return FakeGraph(log)

    sg, impl = StepGraphs(), Impl()
    sg.run('k', impl, ('d', 'g'), capture=capture)
    assert log == []                        # the eager pass touches no planes
    one = [('stale',), ('replay',), ('refresh', 'd', 7), ('refresh', 'g', 7)]
    sg.run('k', impl, ('d', 'g'), capture=capture)
    assert log == one
    gen[0] = 9                              # planes made later: every refresh still gets the generation of the capture
    sg.run('k', impl, ('d', 'g'), capture=capture)
    sg.run('k', impl, ('g', 'd'), capture=capture)
    assert log == one * 2 + [('stale',), ('replay',), ('refresh', 'g', 7), ('refresh', 'd', 7)]
    del log[:]
    sg.run('i', impl, capture=capture)
    sg.run('i', impl, capture=capture)      # no flats (the inference pass): no refresh
    assert log == [('stale',), ('replay',)] and sg.gen == {'k': 7, 'i': 9}


def test_a_custom_capture_and_replay_pair_keeps_its_list():
    played = []

    def capture(impl):
        impl()
        return [('graph', FakeGraph()), ('reduce', 0, 1), ('graph', FakeGraph())]

    def replay(ops):
        assert isinstance(ops, list)
        played.append(ops)
        for op in ops:
            if op[0] == 'graph':
                op[1].replay()

    sg, impl = StepGraphs(), Impl()
    sg.run('k', impl, capture=capture, replay=replay)
    out, ops = sg.run('k', impl, capture=capture, replay=replay)
    assert out == CAPTURED and isinstance(ops, list) and sg.graphs['k'] is ops
    assert sg.run('k', impl, capture=capture, replay=replay) == (REPLAYED, ops)
    assert played == [ops, ops] and [op[1].replays for op in ops if op[0] == 'graph'] == [2, 2]


@pytest.mark.parametrize('label, said', [
    (None, 'hipGraph capture failed'), ('hipGraph capture of the inference pass', 'hipGraph capture of the inference pass failed')])
def test_a_failing_capture_stores_nothing_and_leaves_the_retry_to_the_caller(capsys, monkeypatch, label, said):
    touched = []
    monkeypatch.setattr(hip, 'resplit_stale', lambda: touched.append('stale'))
    monkeypatch.setattr(hip, 'refresh_new_splits', lambda flat, since: touched.append('refresh'))

    def capture(impl):
        raise RuntimeError('capture invalidated')

    sg, impl = StepGraphs(), Impl()
    kw = {} if label is None else {'label': label}
    assert sg.run('k', impl, ('d',), capture=capture, **kw)[0] == EAGER
    capsys.readouterr()
    assert sg.run('k', impl, ('d',), capture=capture, **kw) == (FAILED, None)
    assert impl.calls == 1                  # the eager retry belongs to the caller
    assert sg.graphs == {} and sg.gen == {} and touched == []
    printed = capsys.readouterr().out
    assert printed == "%s (RuntimeError('capture invalidated')): continuing with eager launches\n" % said
