"""GPU: a replay window whose planes are kept as 2-bit codes (agz_replay_create_packed: k_replay_pack_check, k_replay_pack,
k_replay_sample_packed) against an unpacked window of the same rows and against numpy.

Planes are drawn with rng.choice over a palette's bit patterns, policy and value are random normals.  Everything is compared as bytes
(`.tobytes()`): as floats -0.0 == 0.0 and NaN != NaN, which would hide exactly what makes the packing lossless.  The ring is checked
against the last `live` rows the test itself appended, the sampler against tests/test_replay_gpu.py's restatement of the draw and
against k_replay_sample on an unpacked window, the training loop against agz_train_replay on an unpacked window."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_replay_gpu import _trainers, expected_batch

pytestmark = pytest.mark.gpu
INVALID, STATE, UNSUPPORTED = -1, -4, -6
PZ, NZ, ONE, MONE, MILLI, NAN1 = 0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3A83126F, 0x7FC00001
PALETTES = {
    "wq": [PZ, NZ, ONE, MONE],                 # agz_encoder_palette(AGZ_ENC_WQ)
    "twoplane": [MILLI, PZ, ONE, MONE],        # agz_encoder_palette(AGZ_ENC_TWOPLANE)
    "one": [ONE],
    "three": [MILLI, ONE, MONE],
    "negzero-nan": [NZ, NAN1],
}


def pal_floats(name):
    return np.array(PALETTES[name], np.uint32).view(np.float32)


def make_rows(rng, n, F, H, W, A1, pal):
    planes = rng.choice(np.array(PALETTES[pal], np.uint32), size=(n, F * H * W)).astype(np.uint32).view(np.float32)
    return planes, rng.normal(size=(n, A1)).astype(np.float32), rng.normal(size=n).astype(np.float32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Feeder:
    """appends the same rows to every window it holds, by the three routes in turn, and keeps every row ever appended"""

    def __init__(self, ctx, windows, rng, pal):
        self.windows, self.rng, self.pal, self.turn = windows, rng, pal, 0
        rp = windows[0]
        self.shape = (rp.F, rp.H, rp.W, rp.A1)
        self.ex = A.Examples(ctx, *self.shape)
        self.P = np.zeros((0, rp.F * rp.H * rp.W), np.float32)
        self.Q = np.zeros((0, rp.A1), np.float32)
        self.V = np.zeros(0, np.float32)

    def append(self, n, route=None):
        p, q, v = make_rows(self.rng, n, *self.shape, self.pal)
        route = self.turn % 3 if route is None else route
        self.turn += 1
        for rp in self.windows:
            if route == 0:
                rp.append_host(p, q, v)
            else:
                self.ex.clear()
                self.ex.append_host(p, q, v)
                if route == 1:
                    rp.append_dev(*self.ex.raw_dev(), n)
                else:
                    rp.append_examples(self.ex)
                    assert len(self.ex) == n                  # the set is unchanged
        self.P, self.Q, self.V = np.concatenate([self.P, p]), np.concatenate([self.Q, q]), np.concatenate([self.V, v])

    def reset(self):
        self.P, self.Q, self.V = self.P[:0], self.Q[:0], self.V[:0]

    def live(self):
        n = min(len(self.V), self.windows[0].capacity)
        k = len(self.V) - n
        return self.P[k:], self.Q[k:], self.V[k:]

    def close(self):
        self.ex.close()


def check_ring(rp, fd):
    p, q, v = fd.live()
    assert len(rp) == len(v) and rp.total() == len(fd.V)
    gp, gq, gv = rp.get()
    assert same(gp, p) and same(gq, q) and same(gv, v)


@pytest.mark.parametrize("pal", list(PALETTES))
@pytest.mark.parametrize("cap", [5, 7])
def test_ring_keeps_the_last_rows_in_order(ctx, cap, pal):
    rng = np.random.default_rng(100 + cap)
    rp = A.Replay(ctx, 2, 3, 3, 10, cap, palette=pal_floats(pal))
    assert len(rp) == 0 and rp.total() == 0 and rp.capacity == cap and rp.storage()[0] is True
    fd = Feeder(ctx, [rp], rng, pal)
    # 1, 3 and cap - 1 rows by every route, crossing the wrap several times; one append larger than the window and one exactly its size by
    # every route too (the sizes of test_replay_gpu.py::test_ring_keeps_the_last_rows_in_order)
    sizes = [1, 3, cap - 1] * 3 + [cap + 3, cap, 1, cap + 3, cap, 3, cap + 3, cap, cap - 1, 1, 3]
    for n in sizes:
        fd.append(n)
        check_ring(rp, fd)
    assert rp.total() > 8 * cap
    p, q, v = fd.live()
    for j0, cnt in ((0, 1), (1, cap - 1), (cap - 2, 2), (cap, 0)):     # a part of the window that crosses the physical wrap
        gp, gq, gv = rp.get(j0, cnt)
        assert same(gp, p[j0:j0 + cnt]) and same(gq, q[j0:j0 + cnt]) and same(gv, v[j0:j0 + cnt])
    with pytest.raises(A.AgzError):
        rp.get(1, cap)
    rp.clear()
    assert len(rp) == 0 and rp.total() == 0
    fd.reset()
    for n in (2, cap - 1, 3):
        fd.append(n)
        check_ring(rp, fd)
    fd.close()
    rp.close()


def test_a_host_append_longer_than_the_staging_buffer_and_the_window(ctx):
    """append_host sends its rows up through a staging buffer of at most 8 MiB: 322 rows of 19x19 x 18 planes.  700 rows into a window of
    650 that already holds 100: the first 50 are skipped, the rest go up in three chunks, the second of which crosses the physical wrap."""
    F, S, A1, cap, pal = 18, 19, 362, 650, "wq"
    assert 2 * ((8 << 20) // (F * S * S * 4)) < cap
    rng = np.random.default_rng(19)
    rp = A.Replay(ctx, F, S, S, A1, cap, palette=pal_floats(pal))
    fd = Feeder(ctx, [rp], rng, pal)
    fd.append(100, route=0)
    fd.append(700, route=0)
    check_ring(rp, fd)
    assert rp.total() == 800 and len(rp) == cap
    # a bad cell in the last row of such an append: nothing is taken
    p, q, v = make_rows(rng, 700, F, S, S, A1, pal)
    p.view(np.uint32)[699, F * S * S - 1] = MILLI
    assert capi.lib().agz_replay_append_host(rp.h, capi._pf(p), capi._pf(q), capi._pf(v), 700) == INVALID
    assert b"row 699, element %d" % (F * S * S - 1) in capi.lib().agz_last_error()
    check_ring(rp, fd)
    fd.close()
    rp.close()


def test_a_device_append_of_more_rows_than_one_grid_holds(ctx):
    """70 000 rows of 3x3 by the two device routes: more rows than a grid's second dimension (65 535), so k_replay_pack strides over rows,
    and 1.26 M elements, more than k_replay_pack_check's 4096 workgroups hold at once.  Two bad cells far apart: the smaller is named."""
    F, S, A1, n, pal = 2, 3, 10, 70000, "twoplane"
    L = capi.lib()
    rng = np.random.default_rng(70)
    rp = A.Replay(ctx, F, S, S, A1, n + 1, palette=pal_floats(pal))
    fd = Feeder(ctx, [rp], rng, pal)
    fd.append(3, route=0)
    p, q, v = make_rows(rng, n, F, S, S, A1, pal)
    bad = p.copy()
    bad.view(np.uint32)[69990, 17] = NZ
    bad.view(np.uint32)[66000, 4] = NAN1
    ex = A.Examples(ctx, F, S, S, A1)
    ex.append_host(bad, q, v)
    assert L.agz_replay_append_dev(rp.h, *[C.c_void_p(a) for a in ex.raw_dev()], n) == INVALID
    msg = L.agz_last_error()
    assert b"row 66000, element 4 " in msg and b"0x7FC00001" in msg, msg
    assert L.agz_replay_append_examples(rp.h, ex.h) == INVALID
    check_ring(rp, fd)
    fd.append(n, route=1)                                                # wraps: the window keeps the last n + 1 of n + 3 rows
    check_ring(rp, fd)
    fd.append(n, route=2)
    check_ring(rp, fd)
    for h in (ex, rp):
        h.close()
    fd.close()


SAMPLER_CASES = [  # H, W, F, A1, cap, palette
    pytest.param(3, 3, 2, 10, 11, "wq", id="3x3-one-partial-word"),
    pytest.param(4, 4, 3, 17, 11, "negzero-nan", id="4x4-exactly-one-word"),
    pytest.param(5, 5, 3, 26, 11, "three", id="5x5-a-word-and-a-partial-one"),
    pytest.param(6, 7, 2, 8, 11, "twoplane", id="6x7-nonsquare"),
    pytest.param(19, 19, 18, 362, 40, "wq", id="19x19-row-longer-than-a-segment"),
    pytest.param(3, 3, 2, 10, 11, "one", id="3x3-one-entry"),
    pytest.param(5, 5, 3, 26, 11, "twoplane", id="5x5-twoplane"),
]


@pytest.mark.parametrize("H,W,F,A1,cap,pal", SAMPLER_CASES)
def test_sampler_equals_the_unpacked_window_and_the_restatement(ctx, H, W, F, A1, cap, pal):
    rng = np.random.default_rng(7 * H + W + A1)
    packed = A.Replay(ctx, F, H, W, A1, cap, palette=pal_floats(pal))
    plain = A.Replay(ctx, F, H, W, A1, cap)
    fd = Feeder(ctx, [packed, plain], rng, pal)
    out = A.Examples(ctx, F, H, W, A1)                                   # sample_dev's read-back: append_dev / get
    buf = A.Examples(ctx, F, H, W, A1)                                   # device buffers for sample_dev: 257 rows
    buf.append_host(np.zeros((257, F * H * W), np.float32), np.zeros((257, A1), np.float32), np.zeros(257, np.float32))
    bx, bp, bv = buf.raw_dev()
    square = H == W
    if not square:
        fd.append(3)
        L = capi.lib()
        x, p, v = np.zeros((1, F, H, W), np.float32), np.zeros((1, A1), np.float32), np.zeros(1, np.float32)
        assert L.agz_replay_sample(packed.h, 1, 1, 0, 1, capi._pf(x), capi._pf(p), capi._pf(v)) == INVALID     # symmetric = 1 is refused
        assert b"square boards" in L.agz_last_error()
        assert L.agz_replay_sample_dev(packed.h, 1, 1, 0, 1, C.c_void_p(bx), C.c_void_p(bp), C.c_void_p(bv)) == INVALID
        for rp in (packed, plain):
            rp.clear()
        fd.reset()
    seed = 2024 + H
    ks_seen = set()
    for state in ("partly filled", "wrapped"):
        if state == "partly filled":
            fd.append(4)
            fd.append(3)
            assert len(packed) == 7 < cap
        else:
            fd.append(cap - 2)
            fd.append(5)
            assert packed.total() == cap + 10 and len(packed) == cap
        live = fd.live()
        for rows in (1, 3, 64, 257):
            for step in (0, 5):
                for symmetric in ((False, True) if square else (False,)):
                    X, Pi, V, jj, kk = expected_batch(live, seed, step, rows, symmetric, F, H, W, A1)
                    msg = "%s rows %d step %d symmetric %d" % (state, rows, step, symmetric)
                    x, p, v = packed.sample(rows, seed, step, symmetric)
                    assert same(x, X) and same(p, Pi) and same(v, V), msg
                    ux, up, uv = plain.sample(rows, seed, step, symmetric)             # k_replay_sample on the same rows
                    assert same(x, ux) and same(p, up) and same(v, uv), msg
                    packed.sample_dev(rows, seed, step, symmetric, bx, bp, bv)
                    out.clear()
                    out.append_dev(bx, bp, bv, rows)
                    dx, dp, dv = out.get()
                    assert same(dx.reshape(X.shape), X) and same(dp, Pi) and same(dv, V), msg + " (sample_dev)"
                    plain.sample_dev(rows, seed, step, symmetric, bx, bp, bv)
                    out.clear()
                    out.append_dev(bx, bp, bv, rows)
                    ex, ep, ev = out.get()
                    assert same(dx, ex) and same(dp, ep) and same(dv, ev), msg + " (sample_dev, unpacked)"
                    ks_seen |= set(kk.tolist())
    assert ks_seen == (set(range(8)) if square else {0})
    if pal == "negzero-nan":                                               # the NaN entry arrived with its payload, -0.0 with its sign
        assert set(np.unique(x.view(np.uint32)).tolist()) == {NZ, NAN1}
    for h in (buf, out, plain, packed):
        h.close()
    fd.close()


def test_a_bad_cell_refuses_the_whole_append(ctx):
    L = capi.lib()
    F, S, A1, cap, pal = 2, 3, 10, 6, "wq"
    rng = np.random.default_rng(11)
    rp = A.Replay(ctx, F, S, S, A1, cap, palette=pal_floats(pal))
    fd = Feeder(ctx, [rp], rng, pal)
    fd.append(4)
    fd.append(4)                                                         # wrapped: total 8, live 6
    before = [a.copy() for a in rp.get()]
    ex = A.Examples(ctx, F, S, S, A1)

    def refused(p, q, v, where):
        n = len(v)
        ex.clear()
        ex.append_host(p, q, v)
        dp, dq, dv = ex.raw_dev()
        calls = (("agz_replay_append_host", lambda: L.agz_replay_append_host(rp.h, capi._pf(p), capi._pf(q), capi._pf(v), n)),
                 ("agz_replay_append_dev", lambda: L.agz_replay_append_dev(rp.h, C.c_void_p(dp), C.c_void_p(dq), C.c_void_p(dv), n)),
                 ("agz_replay_append_examples", lambda: L.agz_replay_append_examples(rp.h, ex.h)))
        for name, call in calls:
            assert call() == INVALID, name
            msg = L.agz_last_error()
            assert name.encode() in msg and where in msg and b"0x3A83126F" in msg, msg
            assert len(rp) == cap and rp.total() == 8, name
            assert all(same(a, b) for a, b in zip(rp.get(), before)), name

    # the second row of three has one cell outside the palette (and a later row another: the first one is named)
    p, q, v = make_rows(rng, 3, F, S, S, A1, pal)
    p.view(np.uint32)[1, 13] = MILLI
    p.view(np.uint32)[2, 1] = MILLI
    refused(p, q, v, b"row 1, element 13")
    # cap + 3 rows, the bad cell in a row the ring would have skipped
    p, q, v = make_rows(rng, cap + 3, F, S, S, A1, pal)
    p.view(np.uint32)[1, 0] = MILLI
    refused(p, q, v, b"row 1, element 0")
    # -0.0 is not +0.0: a window whose palette holds only +0.0 among the zeros
    tp = A.Replay(ctx, F, S, S, A1, cap, palette=pal_floats("twoplane"))
    p, q, v = make_rows(rng, 2, F, S, S, A1, "twoplane")
    p.view(np.uint32)[0, 5] = NZ
    assert L.agz_replay_append_host(tp.h, capi._pf(p), capi._pf(q), capi._pf(v), 2) == INVALID
    assert b"0x80000000" in L.agz_last_error() and len(tp) == 0
    with pytest.raises(A.AgzError):
        tp.append_host(p, q, v)
    # the window still takes good rows
    fd.append(2)
    check_ring(rp, fd)
    for h in (ex, tp, rp):
        h.close()
    fd.close()


def test_refusals(ctx):
    L = capi.lib()
    F, S, A1 = 2, 3, 10
    out = C.c_void_p()
    five = np.array([0.0, 1.0, -1.0, 0.001, 2.0], np.float32)
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 4, capi._pf(five), 0, C.byref(out)) == INVALID      # n_palette 0 and 5
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 4, capi._pf(five), 5, C.byref(out)) == INVALID
    assert b"palette" in L.agz_last_error()
    dup = np.array([0.0, 1.0, 0.0], np.float32)
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 4, capi._pf(dup), 3, C.byref(out)) == INVALID       # duplicate entries
    assert b"same bit pattern" in L.agz_last_error()
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 4, None, 2, C.byref(out)) == INVALID
    # what agz_replay_create refuses
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 0, capi._pf(five), 4, C.byref(out)) == INVALID      # capacity < 1
    assert L.agz_replay_create_packed(ctx.h, F, S, S, 0, 4, capi._pf(five), 4, C.byref(out)) == INVALID
    assert L.agz_replay_create_packed(ctx.h, F, S, S, A1, 4, capi._pf(five), 4, None) == INVALID
    with pytest.raises(A.AgzError):
        A.Replay(ctx, F, S, S, A1, 4, palette=[0.0, 0.0])
    # +0.0 and -0.0 together are a palette
    pz = A.Replay(ctx, F, S, S, A1, 4, palette=np.array([0.0, -0.0], np.float32))
    pz.close()
    # an empty packed window
    rp = A.Replay(ctx, F, S, S, A1, 6, palette=pal_floats("twoplane"))
    t, = _trainers(ctx, 1, False)
    before = [t.get_param(i) for i in range(t.num_params())]
    cost = C.c_float(0)
    x, p, v = np.zeros((1, F, S, S), np.float32), np.zeros((1, A1), np.float32), np.zeros(1, np.float32)
    assert L.agz_train_replay(t.h, rp.h, 1, 1, 0, C.byref(cost)) == STATE
    assert L.agz_replay_sample(rp.h, 1, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == STATE
    rp.append_host(*make_rows(np.random.default_rng(0), 4, F, S, S, A1, "twoplane"))
    assert L.agz_replay_sample(rp.h, 0, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == INVALID      # rows < 1
    assert L.agz_replay_sample(rp.h, 1, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == 0
    # another shape: the example set's rows must be the window's
    ex = A.Examples(ctx, F, S, S, A1 + 1)
    assert L.agz_replay_append_examples(rp.h, ex.h) == INVALID
    for i, b in enumerate(before):
        assert t.get_param(i).tobytes() == b.tobytes()
    for h in (t, ex, rp):
        h.close()


def test_a_sharded_trainer_is_refused(ctx):
    """a sharded handle of one rank on a real RCCL communicator (the route of test_replay_gpu.py): AGZ_E_UNSUPPORTED, nothing trained"""
    L = capi.lib()
    F, S, A1, B = 2, 3, 10, 8
    rp = A.Replay(ctx, F, S, S, A1, 6, palette=pal_floats("twoplane"))
    rp.append_host(*make_rows(np.random.default_rng(1), 4, F, S, S, A1, "twoplane"))
    comm = A.Comm.init_all([ctx])[0]
    ts = A.Trainer.sharded(ctx, comm, 32, 1, 16, S, S, F, A1, B)
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


def test_storage_reports_the_bytes_allocated(ctx):
    for F, H, W, A1, cap in ((2, 3, 3, 10, 5), (3, 4, 4, 17, 7), (3, 5, 5, 26, 11), (2, 6, 7, 8, 3), (18, 19, 19, 362, 40)):
        mm = H * W
        wpp = (mm + 15) // 16
        packed = A.Replay(ctx, F, H, W, A1, cap, palette=pal_floats("wq"))
        plain = A.Replay(ctx, F, H, W, A1, cap)
        assert packed.storage() == (True, F * wpp * 4 + A1 * 4 + 4, cap * (F * wpp * 4 + A1 * 4 + 4))
        assert plain.storage() == (False, (F * mm + A1 + 1) * 4, cap * (F * mm + A1 + 1) * 4)
        if mm == 361:
            assert packed.storage()[1] == 3108 and plain.storage()[1] == 27444
        # any of the three may be NULL
        L = capi.lib()
        row = C.c_int64(0)
        assert L.agz_replay_storage(packed.h, None, C.byref(row), None) == 0 and row.value == packed.storage()[1]
        assert L.agz_replay_storage(packed.h, None, None, None) == 0
        packed.close()
        plain.close()


ENCODER_CASES = [
    pytest.param(dict(kind=capi.GAME_KOMI, m=5, n=5, k=3, encoder=capi.ENC_WQ), 18, 26, id="komi5x5-wq"),
    pytest.param(dict(kind=capi.GAME_MNK, m=3, n=3, k=3, encoder=capi.ENC_TWOPLANE), 2, 10, id="mnk3x3-twoplane"),
]


@pytest.mark.parametrize("game,F,A1", ENCODER_CASES)
def test_the_encoders_rows_fit_their_palettes(ctx, game, F, A1):
    """complete self-play games on the device (the arenas of test_examples_gpu.py: AGZ_INF_HASH), their examples into a packed window under
    agz_encoder_palette and into an unpacked one: the same bytes come back.  WQ's rows must hold -0.0, or the test shows nothing."""
    S = game["m"]
    arena = A.Arena(ctx, n_games=6, seed=5, Budget=8, **game)
    arena.set_inferencer(0, capi.INF_HASH)
    arena.set_inferencer(1, capi.INF_HASH)
    arena.reset()
    arena.play(0, True)
    ex = A.Examples(ctx, F, S, S, A1)
    ex.append_arena(arena)
    n = len(ex)
    assert n > 6
    pal = capi.encoder_palette(game["encoder"])
    packed = A.Replay(ctx, F, S, S, A1, n + 2, palette=pal)
    plain = A.Replay(ctx, F, S, S, A1, n + 2)
    packed.append_examples(ex)
    plain.append_examples(ex)
    assert len(packed) == len(plain) == n
    got, want, src = packed.get(), plain.get(), ex.get()
    assert all(same(a, b) for a, b in zip(got, want)) and all(same(a, b) for a, b in zip(got, src))
    patterns = set(np.unique(got[0].view(np.uint32)).tolist())
    assert patterns <= set(pal.view(np.uint32).tolist()) and len(patterns) >= 3
    if game["encoder"] == capi.ENC_WQ:
        assert NZ in patterns and PZ in patterns                         # the opponent's empty cells are -0.0
    else:
        assert MILLI in patterns
    x, p, v = packed.sample(64, 3, 0, True)
    ux, up, uv = plain.sample(64, 3, 0, True)
    assert same(x, ux) and same(p, up) and same(v, uv)
    for h in (packed, plain, ex, arena):
        h.close()


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_train_replay_on_a_packed_window_takes_the_steps_of_an_unpacked_one(ctx, adam):
    """agz_train_replay (3 steps, symmetric) on a packed window against the same call on an unpacked window of the same rows, at the shape
    and by the rule of test_replay_gpu.py::test_train_replay_takes_the_steps_of_train_dev_on_the_sampled_minibatches: the unpacked
    reference is run twice; if it is run-to-run bit-reproducible the packed run must equal it bit for bit, parameters and cost, otherwise
    the tolerance is that test's, 1e-4 of a tensor's largest magnitude."""
    F, S, Aspace, B, steps, seed = 2, 3, 10, 8, 3, 4242
    rng = np.random.default_rng(3)
    n = 29                                                             # wrapped
    X = rng.choice(pal_floats("twoplane"), size=(n, F * S * S)).astype(np.float32)
    P = np.zeros((n, Aspace), np.float32)
    P[np.arange(n), rng.integers(0, Aspace, n)] = 1
    V = rng.choice(np.array([-1, 0, 1], np.float32), n).astype(np.float32)
    packed = A.Replay(ctx, F, S, S, Aspace, 20, palette=pal_floats("twoplane"))
    plain = A.Replay(ctx, F, S, S, Aspace, 20)
    for rp in (packed, plain):
        rp.append_host(X[:13], P[:13], V[:13])
        rp.append_host(X[13:], P[13:], V[13:])
    assert all(same(a, b) for a, b in zip(packed.get(), plain.get()))
    ta, tb1, tb2 = _trainers(ctx, 3, adam)
    fresh = [ta.get_param(i) for i in range(ta.num_params())]
    cb1 = tb1.train_replay(plain, steps, seed, True)
    cb2 = tb2.train_replay(plain, steps, seed, True)
    ca = ta.train_replay(packed, steps, seed, True)
    pb1 = [tb1.get_param(i) for i in range(tb1.num_params())]
    pb2 = [tb2.get_param(i) for i in range(tb2.num_params())]
    pa = [ta.get_param(i) for i in range(ta.num_params())]
    reproducible = cb1 == cb2 and all(a.tobytes() == b.tobytes() for a, b in zip(pb1, pb2))
    print("trainer run-to-run bit-reproducible at this shape (adam %d): %s; cost packed %.9g, unpacked %.9g" % (adam, reproducible, ca, cb1))
    assert max(float(np.abs(a - b).max()) for a, b in zip(pa, fresh)) > 0      # training changed the parameters
    if reproducible:
        assert ca == cb1
        for i, (a, b) in enumerate(zip(pa, pb1)):
            assert a.tobytes() == b.tobytes(), ta.param_info(i)
    else:
        assert abs(ca - cb1) <= 1e-4 * max(1.0, abs(cb1))
        for i, (a, b) in enumerate(zip(pa, pb1)):
            assert np.abs(a - b).max() <= 1e-4 * max(np.abs(b).max(), 1e-3), ta.param_info(i)
    for h in (ta, tb1, tb2, packed, plain):
        h.close()
