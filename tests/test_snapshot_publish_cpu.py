"""TrainerServer.publish_network(snapshot) over the loopback transport, with stand-in snapshot objects (no GPU): the call returns
at once and one publisher thread waits, checks, encodes, sends and releases; the queue is one deep and the newest wins; a non-finite
snapshot is never sent; a dict keeps today's synchronous path and today's `stats` keys.  Nothing here sleeps: every hand-over is a
threading.Event."""
import itertools
import logging
import queue
import threading

import numpy as np
import pytest

from serl_amd.transport import TrainerClient, TrainerServer, endpoint, make_trainer_config

_ports = itertools.count(6210, 2)
TIMEOUT = 10.0     # upper bound of every wait below; none is expected to take more than milliseconds


class FakeSnapshot:
    """wait / params / finite / release, as StateSnapshot has them; wait() blocks until `go` is set"""

    def __init__(self, step, finite=True, blocked=False):
        self.step, self._finite = step, finite
        self.nonfinite = {"params": 0 if finite else 2}
        self.go, self.waiting, self.released = threading.Event(), threading.Event(), threading.Event()
        self.params_read = 0
        if not blocked:
            self.go.set()

    def wait(self):
        self.waiting.set()
        assert self.go.wait(TIMEOUT)
        return self

    @property
    def finite(self):
        return self._finite

    @property
    def params(self):
        assert not self.released.is_set()
        self.params_read += 1
        return {"modules_actor": {"w": np.full((3,), self.step, np.float32)}, "step": self.step}

    def release(self):
        assert not self.released.is_set(), "released twice"
        self.released.set()


@pytest.fixture
def session():
    port = next(_ports)
    cfg = make_trainer_config(port_number=port, broadcast_port=port + 1)
    server = TrainerServer(cfg, transport="loopback")
    server.start(threaded=True)
    client = TrainerClient("actor_env", "localhost", cfg, transport="loopback", wait_for_server=True)
    got = queue.Queue()
    client.recv_network_callback(got.put)
    yield server, client, got
    client.stop()
    server.stop()


def test_a_blocked_snapshot_does_not_block_publish_network(session):
    server, _, got = session
    snap = FakeSnapshot(1, blocked=True)
    server.publish_network(snap)            # returns although wait() has not
    assert not snap.go.is_set() and not snap.released.is_set() and server.stats["published"] == 0
    assert snap.waiting.wait(TIMEOUT)       # the publisher thread is the one that waits
    assert threading.current_thread() is not server._pub_thread
    snap.go.set()
    assert got.get(timeout=TIMEOUT)["step"] == 1
    assert snap.released.wait(TIMEOUT)
    assert server.stats["published"] == 1 and snap.params_read == 1


def test_the_newest_wins_and_the_unsent_one_is_released_and_counted(session):
    server, _, got = session
    first, middle, last = FakeSnapshot(1, blocked=True), FakeSnapshot(2), FakeSnapshot(3)
    server.publish_network(first)
    assert first.waiting.wait(TIMEOUT)      # the thread holds `first`; the queue is empty again
    server.publish_network(middle)
    server.publish_network(last)            # replaces `middle` in the queue
    assert middle.released.is_set() and middle.params_read == 0
    assert server.stats["publish_dropped"] == 1
    first.go.set()
    assert [got.get(timeout=TIMEOUT)["step"], got.get(timeout=TIMEOUT)["step"]] == [1, 3]
    assert last.released.wait(TIMEOUT) and first.released.is_set()
    assert server.stats["published"] == 2 and got.empty()


def test_a_nonfinite_snapshot_is_released_not_sent_and_counted(session, caplog):
    server, _, got = session
    bad, good = FakeSnapshot(7, finite=False), FakeSnapshot(8)
    with caplog.at_level(logging.WARNING, logger=endpoint.__name__):
        server.publish_network(bad)
        assert bad.released.wait(TIMEOUT)
        server.publish_network(good)
        assert got.get(timeout=TIMEOUT)["step"] == 8      # the only frame: `bad` went first and sent nothing
    assert bad.params_read == 0 and got.empty()
    assert server.stats["publish_refused_nonfinite"] == 1 and server.stats["published"] == 1
    assert any("step 7" in r.getMessage() and "params" in r.getMessage() for r in caplog.records)


def test_a_dict_is_published_synchronously_with_todays_stats_keys(session):
    server, _, got = session
    tree = {"modules_actor": {"w": np.arange(4, dtype=np.float32)}}
    server.publish_network(tree)
    assert server.stats == {"datastore_msgs": 0, "transitions": 0, "requests": 0, "published": 1}     # sent before the call returned
    assert server._pub_thread is None       # no publisher thread for a session that never hands over a snapshot
    np.testing.assert_array_equal(got.get(timeout=TIMEOUT)["modules_actor"]["w"], tree["modules_actor"]["w"])
    # ... and stays synchronous beside snapshots
    snap = FakeSnapshot(5)
    server.publish_network(snap)
    assert got.get(timeout=TIMEOUT)["step"] == 5 and snap.released.wait(TIMEOUT)
    server.publish_network(tree)
    assert server.stats == {"datastore_msgs": 0, "transitions": 0, "requests": 0, "published": 3}
    assert "modules_actor" in got.get(timeout=TIMEOUT)


def test_stop_releases_a_queued_snapshot_and_joins_the_thread():
    port = next(_ports)
    server = TrainerServer(make_trainer_config(port_number=port, broadcast_port=port + 1), transport="loopback")
    server.start(threaded=True)
    first, queued = FakeSnapshot(1, blocked=True), FakeSnapshot(2)
    server.publish_network(first)
    assert first.waiting.wait(TIMEOUT)
    server.publish_network(queued)
    stopper = threading.Thread(target=server.stop)
    stopper.start()
    assert queued.released.wait(TIMEOUT) and queued.params_read == 0      # stop() released it while the thread was still busy
    first.go.set()                          # lets the thread finish `first`; it then sees the stop flag
    stopper.join(TIMEOUT)
    assert not stopper.is_alive() and not server._pub_thread.is_alive()
    assert first.released.is_set()
    assert server.stats["published"] == 1 and server.stats["publish_dropped"] == 1
    with pytest.raises(RuntimeError):
        server.publish_network(FakeSnapshot(3))


def test_a_failing_encode_releases_the_snapshot_and_the_thread_lives_on(session, monkeypatch):
    server, _, got = session
    real = endpoint.encode

    def failing(msg):
        if isinstance(msg, dict) and msg.get("step") == 1:
            raise ValueError("cannot encode this one")
        return real(msg)
    monkeypatch.setattr(endpoint, "encode", failing)
    doomed, fine = FakeSnapshot(1), FakeSnapshot(2)
    server.publish_network(doomed)
    assert doomed.released.wait(TIMEOUT) and doomed.params_read == 1
    server.publish_network(fine)
    assert got.get(timeout=TIMEOUT)["step"] == 2 and fine.released.wait(TIMEOUT)
    assert server._pub_thread.is_alive() and server.stats["published"] == 1 and server.stats["errors"] == 1


class _Held(RuntimeError):
    status = -3       # what SerlError carries when every slot of the snapshot handle is held


def test_a_callable_is_called_after_the_queued_snapshot_was_released_and_never_fails_the_caller(session):
    server, _, got = session
    first, queued, newest = FakeSnapshot(1, blocked=True), FakeSnapshot(2), FakeSnapshot(3)
    server.publish_network(first)
    assert first.waiting.wait(TIMEOUT)
    server.publish_network(queued)
    seen = []

    def take():
        seen.append(queued.released.is_set())      # the slot of the queued snapshot is free again BEFORE the new one is taken
        return newest
    server.publish_network(take)
    assert seen == [True] and queued.params_read == 0 and server.stats["publish_dropped"] == 1

    def take_with_every_slot_held():
        raise _Held("libserl_mi355 status -3: no free slot")
    server.publish_network(take_with_every_slot_held)      # behind: this network is dropped and counted, the caller goes on
    assert newest.released.is_set() and server.stats["publish_dropped"] == 3      # (`newest` had to give way first)

    def take_that_breaks():
        raise RuntimeError("something else")
    with pytest.raises(RuntimeError, match="something else"):
        server.publish_network(take_that_breaks)
    first.go.set()
    assert got.get(timeout=TIMEOUT)["step"] == 1 and first.released.wait(TIMEOUT)
    last = FakeSnapshot(4)
    server.publish_network(lambda: last)
    assert got.get(timeout=TIMEOUT)["step"] == 4 and last.released.wait(TIMEOUT)
    assert server.stats["published"] == 2 and len(server.encode_seconds) == 2
