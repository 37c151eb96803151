"""The ring and writer thread of the streamed video loop (ssm_amd.video.PassRing) without a GPU: stub events that record their
synchronize(), a list for a writer.  What is pinned is the loop's failure protocol: order, when a slot comes back, what happens after the
writer's first exception, and the shutdown.  Every wait carries a timeout, so a regression fails instead of hanging."""
import queue
import threading

import pytest

from ssm_amd.video import PassRing

WAIT = 10.0          # seconds: far beyond anything a passing run takes


class Event:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def synchronize(self):
        self.log.append(("sync", self.name))


class ListWriter:
    """write_frame appends to `log`; raises `error` on call number `fail_at` (from 1); waits for `gate`, if given, before every frame."""

    def __init__(self, log, fail_at=None, error=None, gate=None):
        self.log, self.fail_at, self.error, self.gate, self.calls = log, fail_at, error, gate, 0
        self.entered = threading.Event()

    def write_frame(self, buf):
        self.calls += 1
        self.entered.set()
        if self.gate is not None:
            assert self.gate.wait(WAIT)
        if self.calls == self.fail_at:
            raise self.error
        self.log.append(("frame", buf))


def take(ring):
    return ring.take(timeout=WAIT)


def bounded(fn):
    """fn() on a thread of its own, joined with a bound: returns what it returns and raises what it raises."""
    box = []

    def call():
        try:
            box.append((fn(), None))
        except BaseException as e:          # noqa: BLE001 - re-raised below
            box.append((None, e))
    t = threading.Thread(target=call, daemon=True)
    t.start()
    t.join(timeout=WAIT)
    assert not t.is_alive(), "the call did not return: the ring hangs"
    if box[0][1] is not None:
        raise box[0][1]
    return box[0][0]


def close(ring):
    bounded(ring.close)
    assert not ring.thread.is_alive(), "close() returned and the writer thread lives"


def test_take_and_hand():
    ring = PassRing(2, ListWriter([]))
    assert sorted((take(ring), take(ring))) == [0, 1]
    with pytest.raises(queue.Empty):
        ring.take(timeout=0)
    ring.hand(1, None, [])
    assert take(ring) == 1
    close(ring)


def test_order_of_slots_rows_and_events():
    log = []
    ring = PassRing(3, ListWriter(log))
    assert ring.thread.daemon and ring.thread.name == "y4m-writer"
    a, b, c = take(ring), take(ring), take(ring)
    ring.hand(None, None, ["first"])                       # an item without a slot or an event: frame 0 of the fixed grid
    ring.hand(b, Event(log, "b"), ["b0", "b1", "b2"])
    ring.hand(a, None, ["a0"])                             # nothing was queued on the GPU for this slot
    ring.hand(c, Event(log, "c"), ["c1", "c0"])
    assert [take(ring) for _ in range(3)] == [b, a, c], "slots come back in the order they were handed over"
    with pytest.raises(queue.Empty):
        ring.take(timeout=0)                               # the item without a slot released none: it was handed over first
    close(ring)
    assert log == [("frame", "first"), ("sync", "b"), ("frame", "b0"), ("frame", "b1"), ("frame", "b2"), ("frame", "a0"),
                   ("sync", "c"), ("frame", "c1"), ("frame", "c0")]


def test_a_slot_is_free_only_after_its_rows_are_written():
    log, gate = [], threading.Event()
    writer = ListWriter(log, gate=gate)
    ring = PassRing(2, writer)
    a, b = take(ring), take(ring)
    ring.hand(a, Event(log, "a"), ["a0", "a1"])
    assert writer.entered.wait(WAIT), "the writer thread never reached the first row"
    with pytest.raises(queue.Empty):
        ring.take(timeout=0)                               # both slots are out and the writer is held inside a's first row
    assert log == [("sync", "a")]
    gate.set()
    assert take(ring) == a
    assert log == [("sync", "a"), ("frame", "a0"), ("frame", "a1")]
    ring.hand(b, None, [])
    assert take(ring) == b
    close(ring)


@pytest.mark.parametrize("m", [1, 3, 4])
def test_a_writer_that_raises_on_its_mth_frame(m):
    log, depth, error = [], 2, RuntimeError("disk full")
    ring = PassRing(depth, ListWriter(log, fail_at=m, error=error))
    settled = []
    ring.settle = lambda: settled.append(len(log))
    n = 0
    for _ in range(2):                                     # two slots of two rows: the m-th frame is in the first or the second
        r = take(ring)
        ring.hand(r, Event(log, n), ["row %d" % n, "row %d" % (n + 1)])
        n += 2
    for _ in range(3 * depth):                             # the producer goes on without blocking: every slot handed over is released
        r = take(ring)
        ring.hand(r, Event(log, n), ["row %d" % n])
        n += 1
    with pytest.raises(RuntimeError) as e:
        close(ring)
    assert e.value is error and ring.failure == [error]
    frames = [x for kind, x in log if kind == "frame"]
    assert frames == ["row %d" % i for i in range(m - 1)], "nothing is written after the exception"
    assert ("sync", 4) not in log, "after a failure the thread no longer waits for events"
    assert settled == [len(log)], "close() settles once, after the thread has ended and before it raises"
    assert sorted(take(ring) for _ in range(depth)) == list(range(depth)), "every slot is back"


def test_an_exception_of_the_producer_goes_first():
    """Leaving the `with` block on an exception shuts the ring down and lets that exception through, not the writer's."""
    log, settled = [], []
    ring = PassRing(2, ListWriter(log, fail_at=1, error=RuntimeError("the writer's")), settle=lambda: settled.append(True))

    def produce():
        with ring:
            ring.hand(take(ring), None, ["row"])
            take(ring), take(ring)                         # the slot came back: the writer has failed by now
            raise KeyError("the producer's")
    with pytest.raises(KeyError, match="the producer's"):
        bounded(produce)
    assert not ring.thread.is_alive() and settled == [True] and len(ring.failure) == 1 and log == []


def test_close_with_nothing_handed_over():
    settled = []
    ring = PassRing(3, ListWriter([]), settle=lambda: settled.append(True))
    close(ring)
    assert settled == [True] and not ring.failure

    def produce():
        with PassRing(1, ListWriter([])) as ring:
            return ring
    assert not bounded(produce).thread.is_alive()
