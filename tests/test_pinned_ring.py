"""pinned_ring.PinnedRing on the host (no GPU): torch.cuda.Event and Tensor.pin_memory are replaced by fakes that keep a log,
as tests/test_bg_batch_cli.py replaces them."""
import pytest
import torch


@pytest.mark.parametrize('shape,dtype,depth', [((3, 5, 5, 3), torch.uint8, 4), ((2, 3), torch.int32, 4), ((7,), torch.float32, 2)])
def test_buffers_come_round_in_order_behind_their_events(monkeypatch, shape, dtype, depth):
    from sketchyscenecolorization_amd.pinned_ring import PinnedRing
    log, pinned = [], []

    class FakeEvent(object):
        def __init__(self):
            self.number = len([e for e in log if e[0] == 'made'])
            log.append(('made', self.number))

        def synchronize(self):
            log.append(('synchronize', self.number))

        def record(self):
            log.append(('record', self.number))

    def fake_pin(self):
        pinned.append(self)
        return self

    monkeypatch.setattr(torch.cuda, 'Event', FakeEvent)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', fake_pin)
    ring = PinnedRing(shape, dtype) if depth == 4 else PinnedRing(shape, dtype, depth=depth)
    assert ring.depth == depth
    handed = []
    for use in range(2 * depth + 1):
        before = len(log)
        buf = ring.next()
        # the buffer's own event was waited for before the buffer came out, and nothing was recorded meanwhile
        assert log[before:][-1] == ('synchronize', use % depth), log[before:]
        assert all(e[0] != 'record' for e in log[before:])
        assert tuple(buf.shape) == tuple(shape) and buf.dtype == dtype and buf.device.type == 'cpu'
        assert any(buf is t for t in pinned), 'the buffer did not go through pin_memory'
        buf.fill_(use % 100)        # written by the caller, as the command line stacks into it
        handed.append(buf)
        before = len(log)
        ring.queued()
        assert log[before:] == [('record', use % depth)]
    # depth buffers, each with an event of its own, used in turn
    assert len(pinned) == depth and len([e for e in log if e[0] == 'made']) == depth
    assert len({b.data_ptr() for b in handed[:depth]}) == depth
    for use, buf in enumerate(handed):
        assert buf is handed[use % depth]
    # every hand-out but a buffer's first follows the record() of its previous use
    for number in range(depth):
        mine = [e[0] for e in log if e[1] == number and e[0] != 'made']
        assert mine[:2] == ['synchronize', 'record'] and all(a != b for a, b in zip(mine, mine[1:])), mine
