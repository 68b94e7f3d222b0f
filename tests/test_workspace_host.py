"""CPU: the owner of the kernels' scratch buffers, ops.workspace / pinned_workspace / workspace_view / workspace_drop, on CPU tensors.  As in
tests/engine_trace.py, ops._stream is replaced by a function that returns a chosen integer, so a 'stream' here is just that number.

Every host thread has its own table {(device, stream, tag): buffer} and its own pins; nothing counts the entries, nothing prunes them, and a
thread's table goes when the thread does."""
import gc
import threading
import weakref

import pytest
import torch

from tcow_amd import _lib, ops


@pytest.fixture
def on(monkeypatch):
    """on(stream): the number ops._stream returns from now on (0 to begin with)."""
    cur = [0]
    monkeypatch.setattr(ops, '_stream', lambda: cur[0])

    def switch(stream):
        cur[0] = stream
    return switch


def ws(nbytes, tag):
    return ops.workspace(nbytes, 'cpu', tag)


def in_thread(fn, *args):
    """fn(*args) on a thread of its own, joined; its result, or its exception raised here."""
    out = []

    def run():
        try:
            out.append((fn(*args), None))
        except BaseException as e:          # noqa: BLE001
            out.append((None, e))
    t = threading.Thread(target=run)
    t.start(); t.join()
    if out[0][1] is not None:
        raise out[0][1]
    return out[0][0]


def ids(view):
    return {stream: id(buf) for stream, buf in view.items()}


def test_identity_and_growth(on):
    a = ws(100, 'host_a')
    assert a.numel() >= 100 and a.dtype == torch.uint8
    assert ws(100, 'host_a') is a and ws(a.numel(), 'host_a') is a and ws(1, 'host_a') is a
    a.fill_(7)
    big = ws(a.numel() + 1, 'host_a')                                    # has to grow: a new tensor, the first one is still its holder's
    assert big is not a and big.numel() >= a.numel() + 1 and big.data_ptr() != a.data_ptr()
    big.fill_(9)
    assert bool((a == 7).all())
    assert ws(100, 'host_a') is big and ws(0, 'host_a') is big           # grow-only; a zero-byte request returns what is there
    on(5)
    other_stream = ws(100, 'host_a')
    assert other_stream is not big and ws(0, 'host_a') is other_stream
    other_tag = ws(100, 'host_b')
    assert other_tag is not other_stream and other_tag is not big
    on(0)
    assert ws(0, 'host_a') is big
    assert ids(ops.workspace_view('host_a')) == {0: id(big), 5: id(other_stream)} and ids(ops.workspace_view('host_b')) == {5: id(other_tag)}


def test_no_eviction_by_count(on):
    a = ws(64, 'a')
    others = [ws(64, 'other%d' % i) for i in range(200)]
    assert ws(64, 'a') is a and ws(0, 'a') is a
    assert all(ws(0, 'other%d' % i) is b for i, b in enumerate(others))


def test_threads_are_apart(on):
    mine = ws(64, 'apart')

    def worker():
        before = ops.workspace_view('apart')
        theirs = ws(64, 'apart')                                         # same stream number, same tag, while `mine` is held
        return before, theirs, ops.workspace_view('apart')
    before, theirs, after = in_thread(worker)
    assert before == {} and theirs is not mine and theirs.data_ptr() != mine.data_ptr()
    assert ids(after) == {0: id(theirs)}
    assert ids(ops.workspace_view('apart')) == {0: id(mine)} and ws(0, 'apart') is mine


def test_a_threads_scratch_dies_with_it(on):
    kept = ws(64, 'mortal'), ws(64, 'bystander')
    views = ids(ops.workspace_view('mortal')), ids(ops.workspace_view('bystander'))

    def worker():
        return weakref.ref(ws(4096, 'mortal'))
    refs = [in_thread(worker) for _ in range(100)]                       # one after the other
    gc.collect()
    assert all(ref() is None for ref in refs)
    assert (ids(ops.workspace_view('mortal')), ids(ops.workspace_view('bystander'))) == views
    assert ws(0, 'mortal') is kept[0] and ws(0, 'bystander') is kept[1]


def test_concurrent_first_use(on):
    gate = threading.Barrier(8)
    views, errs = {}, []

    def worker(i):
        try:
            gate.wait()
            bufs = [ws(32, 'first%d_%d' % (i, j)) for j in range(64)]
            views[i] = [ops.workspace_view('first%d_%d' % (i, j)) for j in range(64)], bufs
        except BaseException as e:          # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs, errs
    assert sorted(views) == list(range(8))
    for per_tag, bufs in views.values():
        assert len(per_tag) == 64 and all(list(v) == [0] and v[0] is b for v, b in zip(per_tag, bufs))
    assert len({b.data_ptr() for _, bufs in views.values() for b in bufs}) == 8 * 64     # all held: all distinct
    assert ops.workspace_view('first0_0') == {}                          # and none of it in this thread


def test_pins(on):
    plain = ws(64, 'pin')
    buf, inner = ws(200, 'pin_src').narrow(0, 0, 200), ws(300, 'pin_src2').narrow(0, 0, 300)
    with ops.pinned_workspace('pin', buf) as got:
        assert got is buf
        for stream in (0, 3, 11):
            on(stream)
            assert ws(200, 'pin') is buf and ws(0, 'pin') is buf
        on(0)
        with pytest.raises(_lib.TcowError) as e:
            ws(201, 'pin')
        assert str(e.value) == "workspace('pin'): the pinned buffer holds 200 bytes, 201 are needed"
        assert ws(64, 'pin_other') is not buf                            # another tag is not pinned
        assert in_thread(lambda: ws(64, 'pin') is not buf and ws(201, 'pin').numel() >= 201)     # nor is this tag in another thread
        with ops.pinned_workspace('pin', inner):
            assert ws(300, 'pin') is inner
        assert ws(200, 'pin') is buf                                     # the nested pin restored the outer one
    assert ws(64, 'pin') is plain                                        # and the outer one the unpinned buffer
    assert ids(ops.workspace_view('pin')) == {0: id(plain)}              # pins never enter the table

    def pin_elsewhere():
        with ops.pinned_workspace('pin', buf):
            return ws(0, 'pin') is buf
    assert in_thread(pin_elsewhere) and ws(64, 'pin') is plain


def test_workspace_drop(on):
    on(1); d1, k1 = ws(64, 'drop'), ws(64, 'keep')
    on(2); d2, k2 = ws(64, 'drop'), ws(64, 'keep')
    theirs = {}
    ready, done = threading.Event(), threading.Event()

    def worker():
        theirs['buf'] = ws(64, 'drop')
        ready.set(); done.wait()
        theirs['after'] = ops.workspace_view('drop')
    t = threading.Thread(target=worker)
    t.start(); ready.wait()
    ops.workspace_drop('drop')
    done.set(); t.join()
    assert ops.workspace_view('drop') == {} and ids(ops.workspace_view('keep')) == {1: id(k1), 2: id(k2)}
    assert ids(theirs['after']) == {2: id(theirs['buf'])}                # another thread's buffers under the tag stay
    fresh = ws(64, 'drop')
    assert fresh is not d1 and fresh is not d2 and ids(ops.workspace_view('drop')) == {2: id(fresh)}
    ops.workspace_drop('never_used')                                     # nothing to forget is no error
