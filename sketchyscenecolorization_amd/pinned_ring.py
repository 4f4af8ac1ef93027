"""A few pinned host buffers of one shape used in turn, for uploads that the host does not wait for: pinning a fresh array
costs milliseconds a time, and a copy from pageable memory returns only when it has happened.  A buffer is written again only
when the copy that last read it has happened: each has an event, recorded behind that copy (``queued``) and waited for before
the buffer is handed out again (``next``).    buf = ring.next(); buf.copy_(v); static.copy_(buf, non_blocking=True); ring.queued()"""
import torch


class PinnedRing(object):
    def __init__(self, shape, dtype, depth=4):
        self.shape, self.dtype, self.depth = tuple(shape), dtype, depth
        self.slots, self.turn = [], -1      # (buffer, event), made when their turn first comes

    def next(self):
        """The next buffer in turn, free to be written."""
        self.turn += 1
        if len(self.slots) < self.depth:
            self.slots.append((torch.empty(self.shape, dtype=self.dtype).pin_memory(), torch.cuda.Event()))
        buf, ev = self.slots[self.turn % self.depth]
        ev.synchronize()        # (an event that was never recorded does not wait)
        return buf

    def queued(self):
        """The copy that reads the buffer handed out last has been queued on the current stream."""
        self.slots[self.turn % self.depth][1].record()
