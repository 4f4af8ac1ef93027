"""hipGraph replay of a step shape, one state machine for GanTrainer's D-/G-steps, its inference pass and BGTrainer's steps.
What a step IS (segments, reducers, Adam, what it returns) stays with the trainers."""
import torch

from . import hip

EAGER, CAPTURED, REPLAYED, FAILED = 'eager', 'captured', 'replayed', 'failed'


def _capture(impl):
    g = hip.new_graph()
    # thread_local: another thread's event polling (the RCCL watchdog) must not invalidate the capture
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        impl()
    return g


class StepGraphs:
    def __init__(self):
        self.graphs, self.seen = {}, set()      # key -> captured object; keys that ran eagerly once
        self.gen = {}                           # key -> hip.split_generation() at its capture

    def run(self, key, impl, flats=(), capture=_capture, replay=None, label='hipGraph capture'):
        """One pass of step ``key``; ``impl()`` reads static tensors only and issues the launches.  EAGER the first time a key is
        seen (the pass allocates buffers and sets kernel attributes), CAPTURED -- ``capture(impl)`` -> the object to keep -- and
        replayed the second time, REPLAYED from then on (``replay(obj)``; default: obj.replay()).  FAILED: the capture raised;
        nothing is stored and impl() has NOT run -- the caller turns its graphs off (no capture is tried again), resets its
        state and runs the step eagerly.  Returns (outcome, captured object or None)."""
        g = self.graphs.get(key)
        outcome = REPLAYED
        if g is None:
            if key not in self.seen:
                self.seen.add(key)
                impl()
                return EAGER, None
            try:
                g = capture(impl)
            except Exception as e:
                print('%s failed (%r): continuing with eager launches' % (label, e))
                return FAILED, None
            self.graphs[key], self.gen[key] = g, hip.split_generation()
            outcome = CAPTURED
        # a replayed graph holds the bf16 planes' addresses and never meets hip.filter_split: weights replaced through torch since
        # the last launch are split again in front of the replay; filters of ``flats`` (the parameter buffers the step's optimizer
        # writes) that met their first bf16 launch after the capture are not in its refresh and are split behind it
        hip.resplit_stale()
        replay(g) if replay else g.replay()
        for flat in flats:
            hip.refresh_new_splits(flat, self.gen[key])
        return outcome, g
