"""The one staging ring of the Python hosts: host blocks the GPU may still be reading."""
import torch


class PinnedRing:
    """``slots`` pinned host blocks behind asynchronous H2D copies.  ``acquire()`` advances to the next slot, waits for the event recorded
    behind that slot's last copy (``slots`` uses ago) and returns its block; the caller fills it, queues its copy and calls ``commit(stream)``,
    which records the slot's event behind that copy.  This order is what keeps batch i+1's bytes out of batch i's queued copy when the host
    never synchronises otherwise.  Events are created at a slot's first commit, so the first ``slots`` uses never wait.  ``pin=False`` with
    one slot serves dry-run and CPU plans; ``event`` is the event type (a fake in CPU tests)."""

    def __init__(self, shape, dtype, slots, pin=True, event=torch.cuda.Event):
        self.blocks = [torch.zeros(shape, dtype=dtype) for _ in range(slots)]
        if pin:
            self.blocks = [b.pin_memory() for b in self.blocks]
        self.events = [None] * slots
        self.slot = slots - 1
        self._event = event

    def acquire(self):
        self.slot = (self.slot + 1) % len(self.blocks)
        if self.events[self.slot] is not None:
            self.events[self.slot].synchronize()
        return self.blocks[self.slot]

    def commit(self, stream):
        ev = self.events[self.slot] = self.events[self.slot] or self._event()
        ev.record(stream)
