"""The ranks of a multi-rank run as threads of the test process (test infrastructure; with jl_comm_create_inproc every exchange is
device copies between the ranks' buffers on one GPU)."""
import threading
import time


def ranks_in_threads(world, body, limit=120.0):
    """body(rank) in one thread per rank; re-raises the first failure.  The threads are daemon threads and share one time limit
    (seconds, sized to the small cases of the tests): a rank that is still running when it ends fails the test instead of holding
    it — a rank whose peer failed waits in a barrier for ever."""
    errs = [None] * world
    outs = [None] * world

    def run(r):
        try:
            outs[r] = body(r)
        except BaseException as e:   # noqa: BLE001 - reported below
            errs[r] = e

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    end = time.monotonic() + limit
    for t in th:
        t.join(max(0.0, end - time.monotonic()))
    for e in errs:
        if e is not None:
            raise e
    alive = [r for r, t in enumerate(th) if t.is_alive()]
    assert not alive, "ranks %s still running after %.0f s" % (alive, limit)
    return outs
