"""One request at a time per engine (host only: no torch, no GPU import).

A DeviceEngine and the native handle under it are single-threaded: per-handle scratch, the pending state of split calls, the
lazily bound tables and the Retriever's pinned result buffers all belong to the one request that is running.  A server runs
its routes on a thread pool, so the facades (Retriever, BM25, Reranker) take the engine's re-entrant lock for the WHOLE of
every public call that reaches the engine -- from the first lazy bind or enqueue to the last read of a pinned buffer or device
result.  Raw DeviceEngine methods take nothing: they are the single-threaded layer under the facades.

    @serialised           a method runs under self.engine.lock (or, for an object that has no engine, its own self.lock);
                          a generator method holds the lock from its first next() to exhaustion, close() or an exception
    lock_of(obj)          that lock
    is_serialised(fn)     whether a function went through the decorator (the marker attribute SERIALISED)

The lock is a threading.RLock: a locked method may call another one on the same thread; it belongs to the thread that took it,
so a generator must be finished or closed on the thread that started it, and a helper thread of a locked call (the writer of
batch_search_to_file) never takes it.
"""
import functools
import inspect

SERIALISED = "__msr_serialised__"


def lock_of(obj):
    """The lock a call on `obj` runs under: its engine's, else its own.  AttributeError when it has neither."""
    lock = getattr(getattr(obj, "engine", None), "lock", None)
    return obj.lock if lock is None else lock


def serialised(fn):
    if inspect.isgeneratorfunction(fn):
        @functools.wraps(fn)
        def run(self, *args, **kwargs):
            # a generator: nothing runs before the first next(); the with statement ends on exhaustion, on close() (GeneratorExit
            # arrives at the yield) and on an exception, thrown in or raised by the body
            with lock_of(self):
                return (yield from fn(self, *args, **kwargs))
    else:
        @functools.wraps(fn)
        def run(self, *args, **kwargs):
            with lock_of(self):
                return fn(self, *args, **kwargs)
    setattr(run, SERIALISED, True)
    return run


def is_serialised(fn):
    return bool(getattr(fn, SERIALISED, False))
