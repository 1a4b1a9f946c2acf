"""GPU: the replay window (agz_replay: device ring, k_replay_sample, agz_train_replay) against numpy.

Rows are random normal floats, so no two cells are equal and a wrong source index shows.  Everything is compared bit for bit with numpy
fancy indexing over the rows the test itself appended: the ring against the last `live` rows, the sampler against the restatement of the
draw in tests/test_replay_cpu.py (Python integers) with the eight maps of agz_symmetry_map, the training loop against agz_train_dev over
the same minibatches sampled to the host."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_replay_cpu import draw_py

pytestmark = pytest.mark.gpu
INVALID, STATE, UNSUPPORTED = -1, -4, -6


def make_rows(rng, n, F, H, W, A1):
    return (rng.normal(size=(n, F * H * W)).astype(np.float32), rng.normal(size=(n, A1)).astype(np.float32),
            rng.normal(size=n).astype(np.float32))


class Feeder:
    """appends rows to a window by the three routes in turn and keeps every row ever appended"""

    def __init__(self, ctx, rp, rng):
        self.rp, self.rng, self.turn = rp, rng, 0
        self.ex = A.Examples(ctx, rp.F, rp.H, rp.W, rp.A1)
        self.P = np.zeros((0, rp.F * rp.H * rp.W), np.float32)
        self.Q = np.zeros((0, rp.A1), np.float32)
        self.V = np.zeros(0, np.float32)

    def append(self, n, route=None):
        rp = self.rp
        p, q, v = make_rows(self.rng, n, rp.F, rp.H, rp.W, rp.A1)
        route = self.turn % 3 if route is None else route
        self.turn += 1
        if route == 0:
            rp.append_host(p, q, v)
        else:
            self.ex.clear()
            self.ex.append_host(p, q, v)
            if route == 1:
                rp.append_dev(*self.ex.raw_dev(), n)
            else:
                rp.append_examples(self.ex)
                assert len(self.ex) == n                      # the set is unchanged
        self.P, self.Q, self.V = np.concatenate([self.P, p]), np.concatenate([self.Q, q]), np.concatenate([self.V, v])

    def live(self):
        n = min(len(self.V), self.rp.capacity)
        k = len(self.V) - n
        return self.P[k:], self.Q[k:], self.V[k:]

    def close(self):
        self.ex.close()


def check_ring(rp, fd):
    p, q, v = fd.live()
    assert len(rp) == len(v) and rp.total() == len(fd.V)
    gp, gq, gv = rp.get()
    np.testing.assert_array_equal(gp, p)
    np.testing.assert_array_equal(gq, q)
    np.testing.assert_array_equal(gv, v)


@pytest.mark.parametrize("cap", [5, 7])
def test_ring_keeps_the_last_rows_in_order(ctx, cap):
    rng = np.random.default_rng(100 + cap)
    rp = A.Replay(ctx, 2, 3, 3, 10, cap)
    assert len(rp) == 0 and rp.total() == 0 and rp.capacity == cap
    fd = Feeder(ctx, rp, rng)
    # 1, 3 and cap - 1 rows by every route, crossing the wrap several times; one append larger than the window and one exactly its size by
    # every route too
    sizes = [1, 3, cap - 1] * 3 + [cap + 3, cap, 1, cap + 3, cap, 3, cap + 3, cap, cap - 1, 1, 3]
    for n in sizes:
        fd.append(n)
        check_ring(rp, fd)
    assert rp.total() > 8 * cap
    # a part of the window that crosses the physical wrap
    p, q, v = fd.live()
    for j0, cnt in ((0, 1), (1, cap - 1), (cap - 2, 2), (cap, 0)):
        gp, gq, gv = rp.get(j0, cnt)
        np.testing.assert_array_equal(gp, p[j0:j0 + cnt])
        np.testing.assert_array_equal(gq, q[j0:j0 + cnt])
        np.testing.assert_array_equal(gv, v[j0:j0 + cnt])
    with pytest.raises(A.AgzError):
        rp.get(1, cap)
    with pytest.raises(A.AgzError):
        rp.get(-1, 1)
    rp.clear()
    assert len(rp) == 0 and rp.total() == 0
    fd.P, fd.Q, fd.V = fd.P[:0], fd.Q[:0], fd.V[:0]
    for n in (2, cap - 1, 3):
        fd.append(n)
        check_ring(rp, fd)
    fd.close()
    rp.close()


def expected_batch(live, seed, step, rows, symmetric, F, H, W, A1):
    p, q, v = live
    d = draw_py(seed, step, rows, len(v), symmetric)
    jj = np.array([x[0] for x in d], np.int64)
    kk = np.array([x[1] for x in d], np.int64)
    mm = H * W
    if H == W:
        maps = np.stack([capi.symmetry_map(H, k) for k in range(8)]).astype(np.int64)
        idx = maps[kk]                                                   # [rows, mm]: the source cell of every output cell
    else:
        assert not kk.any()
        idx = np.broadcast_to(np.arange(mm), (rows, mm))
    X = np.take_along_axis(p[jj].reshape(rows, F, mm), idx[:, None, :], axis=2).reshape(rows, F, H, W)
    Pi = q[jj].copy()
    if H == W:                                                           # (a non-square board's policy row is copied: it may be shorter than the board)
        Pi[:, :mm] = np.take_along_axis(q[jj][:, :mm], idx, axis=1)
    return X, Pi, v[jj], jj, kk


SAMPLER_CASES = [  # m or (H, W), F, A1, cap
    pytest.param(3, 3, 2, 10, 11, id="3x3-tail1"),
    pytest.param(5, 5, 3, 26, 11, id="5x5"),
    pytest.param(5, 5, 3, 25, 11, id="5x5-notail"),
    pytest.param(19, 19, 18, 362, 40, id="19x19-row-longer-than-a-segment"),
    pytest.param(6, 7, 2, 8, 11, id="6x7-nonsquare"),
]


@pytest.mark.parametrize("H,W,F,A1,cap", SAMPLER_CASES)
def test_sampler_equals_the_restatement(ctx, H, W, F, A1, cap):
    rng = np.random.default_rng(7 * H + W + A1)
    rp = A.Replay(ctx, F, H, W, A1, cap)
    fd = Feeder(ctx, rp, rng)
    out = A.Examples(ctx, F, H, W, A1)                                   # sample_dev's read-back: append_dev / get
    buf = A.Examples(ctx, F, H, W, A1)                                   # device buffers for sample_dev: 257 rows
    buf.append_host(*[np.zeros_like(a) for a in make_rows(rng, 257, F, H, W, A1)])
    bx, bp, bv = buf.raw_dev()
    square = H == W
    if not square:
        fd.append(3)
        L = capi.lib()
        x, p, v = np.zeros((1, F, H, W), np.float32), np.zeros((1, A1), np.float32), np.zeros(1, np.float32)
        assert L.agz_replay_sample(rp.h, 1, 1, 0, 1, capi._pf(x), capi._pf(p), capi._pf(v)) == INVALID     # symmetric = 1 is refused
        assert b"square boards" in L.agz_last_error()
        assert L.agz_replay_sample_dev(rp.h, 1, 1, 0, 1, C.c_void_p(bx), C.c_void_p(bp), C.c_void_p(bv)) == INVALID
        rp.clear()
        fd.P, fd.Q, fd.V = fd.P[:0], fd.Q[:0], fd.V[:0]
    seed = 2024 + H
    ks_seen = set()
    for state in ("partly filled", "wrapped"):
        if state == "partly filled":
            fd.append(4)
            fd.append(3)
            assert len(rp) == 7 < cap
        else:
            fd.append(cap - 2)
            fd.append(5)
            assert rp.total() == cap + 10 and len(rp) == cap
        live = fd.live()
        for rows in (1, 3, 64, 257):
            for step in (0, 5):
                got = {}
                for symmetric in ((False, True) if square else (False,)):
                    X, Pi, V, jj, kk = expected_batch(live, seed, step, rows, symmetric, F, H, W, A1)
                    msg = "%s rows %d step %d symmetric %d" % (state, rows, step, symmetric)
                    x, p, v = rp.sample(rows, seed, step, symmetric)
                    np.testing.assert_array_equal(x, X, err_msg=msg)
                    np.testing.assert_array_equal(p, Pi, err_msg=msg)
                    np.testing.assert_array_equal(v, V, err_msg=msg)
                    x2, p2, v2 = rp.sample(rows, seed, step, symmetric)             # the same arguments: the same bits
                    assert x2.tobytes() == x.tobytes() and p2.tobytes() == p.tobytes() and v2.tobytes() == v.tobytes(), msg
                    rp.sample_dev(rows, seed, step, symmetric, bx, bp, bv)
                    out.clear()
                    out.append_dev(bx, bp, bv, rows)
                    dx, dp, dv = out.get()
                    np.testing.assert_array_equal(dx.reshape(X.shape), X, err_msg=msg + " (sample_dev)")
                    np.testing.assert_array_equal(dp, Pi, err_msg=msg + " (sample_dev)")
                    np.testing.assert_array_equal(dv, V, err_msg=msg + " (sample_dev)")
                    got[symmetric] = v
                    ks_seen |= set(kk.tolist())
                if square:
                    np.testing.assert_array_equal(got[False], got[True])            # on and off draw the same rows
    assert ks_seen == (set(range(8)) if square else {0})
    for h in (buf, out):
        h.close()
    fd.close()
    rp.close()


def _trainers(ctx, n, adam):
    K, L, FC, S, F, Aspace, B = 32, 1, 16, 3, 2, 10, 8               # test_examples_gpu.py::test_train_dev_matches_host_train's shape
    ts = [A.Trainer(ctx, K, L, FC, S, S, F, Aspace, B) for _ in range(n)]
    for t in ts:
        t.init_random(9)
        if adam:
            t.set_adam()
    return ts


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_train_replay_takes_the_steps_of_train_dev_on_the_sampled_minibatches(ctx, adam):
    """agz_train_replay(steps = 3) against agz_train_dev(batches = 3, iterations = 1) over the three minibatches sampled to the host and
    stacked in step order (iteration 0 of agz_train_dev takes its batches in order): the same kernels on the same data.  The reference is
    run twice first; if the trainer is run-to-run bit-reproducible at this shape the replay run must equal it bit for bit, parameters and
    cost.  If it is not (the BatchNorm sums and the weight gradient accumulate with atomics), the tolerance is the one
    test_examples_gpu.py::test_train_dev_matches_host_train uses for two routes to the same steps: 1e-4 of a tensor's largest magnitude."""
    F, S, Aspace, B, steps, seed = 2, 3, 10, 8, 3, 4242
    rng = np.random.default_rng(3)
    rp = A.Replay(ctx, F, S, S, Aspace, 20)
    n = 29                                                             # wrapped
    X = rng.choice(np.array([0.0, 1.0], np.float32), size=(n, F * S * S)).astype(np.float32)
    P = np.zeros((n, Aspace), np.float32)
    P[np.arange(n), rng.integers(0, Aspace, n)] = 1
    V = rng.choice(np.array([-1, 0, 1], np.float32), n).astype(np.float32)
    rp.append_host(X[:13], P[:13], V[:13])
    rp.append_host(X[13:], P[13:], V[13:])
    mb = [rp.sample(B, seed, step, True) for step in range(steps)]
    ex = A.Examples(ctx, F, S, S, Aspace)
    ex.append_host(np.concatenate([m[0] for m in mb]), np.concatenate([m[1] for m in mb]), np.concatenate([m[2] for m in mb]))
    xd, pd, vd = ex.raw_dev()
    ta, tb1, tb2 = _trainers(ctx, 3, adam)
    cb1 = tb1.train_dev(xd, pd, vd, steps, 1, seed=5)
    cb2 = tb2.train_dev(xd, pd, vd, steps, 1, seed=5)
    ca = ta.train_replay(rp, steps, seed, True)
    pb1 = [tb1.get_param(i) for i in range(tb1.num_params())]
    pb2 = [tb2.get_param(i) for i in range(tb2.num_params())]
    pa = [ta.get_param(i) for i in range(ta.num_params())]
    reproducible = cb1 == cb2 and all(a.tobytes() == b.tobytes() for a, b in zip(pb1, pb2))
    print("trainer run-to-run bit-reproducible at this shape (adam %d): %s; cost replay %.9g, train_dev %.9g" % (adam, reproducible, ca, cb1))
    assert max(float(np.abs(a - b).max()) for a, b in zip(pa, _fresh_params(ctx))) > 0      # training changed the parameters
    if reproducible:
        assert ca == cb1
        for i, (a, b) in enumerate(zip(pa, pb1)):
            assert a.tobytes() == b.tobytes(), ta.param_info(i)
    else:
        assert abs(ca - cb1) <= 1e-4 * max(1.0, abs(cb1))
        for i, (a, b) in enumerate(zip(pa, pb1)):
            assert np.abs(a - b).max() <= 1e-4 * max(np.abs(b).max(), 1e-3), ta.param_info(i)
    assert ta.train_replay(rp, 0, seed, True) == 0.0                   # no step: nothing happens
    for i, a in enumerate(pa):
        assert ta.get_param(i).tobytes() == a.tobytes()
    for h in (ta, tb1, tb2, ex, rp):
        h.close()


def _fresh_params(ctx):
    t, = _trainers(ctx, 1, False)
    ps = [t.get_param(i) for i in range(t.num_params())]
    t.close()
    return ps


def test_refusals(ctx):
    L = capi.lib()
    F, S, Aspace, B = 2, 3, 10, 8
    out = C.c_void_p()
    assert L.agz_replay_create(ctx.h, F, S, S, Aspace, 0, C.byref(out)) == INVALID      # capacity < 1
    assert L.agz_replay_create(ctx.h, F, S, S, 0, 4, C.byref(out)) == INVALID
    rp = A.Replay(ctx, F, S, S, Aspace, 6)
    t, = _trainers(ctx, 1, False)
    before = [t.get_param(i) for i in range(t.num_params())]
    cost = C.c_float(0)
    x, p, v = np.zeros((1, F, S, S), np.float32), np.zeros((1, Aspace), np.float32), np.zeros(1, np.float32)
    # an empty window
    assert L.agz_train_replay(t.h, rp.h, 1, 1, 0, C.byref(cost)) == STATE
    assert L.agz_replay_sample(rp.h, 1, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == STATE
    rng = np.random.default_rng(0)
    rp.append_host(*make_rows(rng, 4, F, S, S, Aspace))
    assert L.agz_replay_sample(rp.h, 0, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == INVALID      # rows < 1
    assert L.agz_train_replay(t.h, rp.h, -1, 1, 0, C.byref(cost)) == INVALID
    # a policy row shorter than the board: no symmetric sampling
    short = A.Replay(ctx, F, S, S, S * S - 1, 6)
    short.append_host(*make_rows(rng, 2, F, S, S, S * S - 1))
    xs, ps = np.zeros((1, F, S, S), np.float32), np.zeros((1, S * S - 1), np.float32)
    assert L.agz_replay_sample(short.h, 1, 1, 0, 1, capi._pf(xs), capi._pf(ps), capi._pf(v)) == INVALID
    assert b"policy shorter than the board" in L.agz_last_error()
    assert L.agz_replay_sample(short.h, 1, 1, 0, 0, capi._pf(xs), capi._pf(ps), capi._pf(v)) == 0
    # another shape: window and trainer, window and example set
    other = A.Replay(ctx, F, S, S, Aspace + 1, 6)
    other.append_host(*make_rows(rng, 2, F, S, S, Aspace + 1))
    assert L.agz_train_replay(t.h, other.h, 1, 1, 0, C.byref(cost)) == INVALID
    ex = A.Examples(ctx, F, S, S, Aspace)
    ex.append_host(*make_rows(rng, 2, F, S, S, Aspace))
    assert L.agz_replay_append_examples(other.h, ex.h) == INVALID
    assert other.total() == 2
    # another context
    ctx2 = A.Ctx(0)
    rp2 = A.Replay(ctx2, F, S, S, Aspace, 6)
    rp2.append_host(*make_rows(rng, 3, F, S, S, Aspace))
    assert L.agz_train_replay(t.h, rp2.h, 1, 1, 0, C.byref(cost)) == INVALID
    assert b"different contexts" in L.agz_last_error()
    assert L.agz_replay_append_examples(rp2.h, ex.h) == INVALID
    rp2.close()
    ctx2.close()
    # nothing above trained
    for i, b in enumerate(before):
        assert t.get_param(i).tobytes() == b.tobytes()
    for h in (t, ex, other, short, rp):
        h.close()


def test_a_sharded_trainer_is_refused(ctx):
    """a sharded handle of one rank on a real RCCL communicator (the route of test_comm_gpu.py): AGZ_E_UNSUPPORTED, nothing trained"""
    L = capi.lib()
    F, S, Aspace, B = 2, 3, 10, 8
    rp = A.Replay(ctx, F, S, S, Aspace, 6)
    rp.append_host(*make_rows(np.random.default_rng(1), 4, F, S, S, Aspace))
    comm = A.Comm.init_all([ctx])[0]
    ts = A.Trainer.sharded(ctx, comm, 32, 1, 16, S, S, F, Aspace, B)
    ts.init_random(9)
    before = [ts.get_param(i) for i in range(ts.num_params())]
    cost = C.c_float(0)
    assert L.agz_train_replay(ts.h, rp.h, 1, 1, 0, C.byref(cost)) == UNSUPPORTED
    assert b"sharded" in L.agz_last_error()
    for i, b in enumerate(before):
        assert ts.get_param(i).tobytes() == b.tobytes()
    ts.close()
    comm.close()
    rp.close()
