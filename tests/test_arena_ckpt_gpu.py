"""GPU: agz_arena_save / agz_arena_load — a saved arena continues bit for bit.

The pattern throughout: arena U plays 2N moves uninterrupted; arena S plays N moves, saves and is destroyed; arena L is created with a
DIFFERENT seed, gets its inferencers (lanes, pool policy) set again, loads, and plays N moves.  After every one of those moves L equals U:
boards, agz_game_state and histories of every game, both agents' root children (moves, visits, blackScores bits, prior bits) and node
counts, the statistics, the results, all sixteen debug counters, and every example row with its game index (compared per game: the row order
among the games of ONE move is the order of an atomic counter).  Refused files and refused saves leave the arena equal to an untouched twin.
Nothing here depends on timing, the oracle or the reference."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi

pytestmark = pytest.mark.gpu

E_INVALID, E_NOMEM, E_STATE = -1, -3, -4
CELLS_PAD, RING = 384, 8

C4 = dict(kind=capi.GAME_C4, m=6, n=7, k=4, n_games=8, Budget=16)
WQ9 = dict(kind=capi.GAME_WQ, m=9, n=9, komi=5.5, encoder=capi.ENC_WQ, n_games=6, Budget=48, RandomCount=4)
KOMI5 = dict(kind=capi.GAME_KOMI, m=5, n=5, k=3, n_games=4, Budget=32)
WQ7 = dict(kind=capi.GAME_WQ, m=7, n=7, komi=5.5, encoder=capi.ENC_WQ, n_games=8, Budget=24)


def make(ctx, conf, seed, inf=capi.INF_HASH, net=None, lanes=1, policy=None, staging=None, **over):
    c = dict(conf, **over)
    a = A.Arena(ctx, c.pop("kind"), c.pop("m"), c.pop("n"), seed=seed, **c)
    if lanes > 1:
        a.set_parallel(lanes)
    for agent in (0, 1):
        a.set_inferencer(agent, inf, net)
    if policy is not None:
        a.set_pool_policy(policy)
    if staging is not None:
        a.set_ckpt_staging(staging)
    return a


def move(a, record=True):
    a.begin_move()
    a.simulate(a.mconf.Budget)
    a.end_move(record)


def counters(a):
    out = []
    for k in range(16):
        v = C.c_int64(0)
        assert capi.lib().agz_arena_debug_counter(a.h, k, C.byref(v)) == 0
        out.append(v.value)
    return out


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def snapshot(a):
    """everything the public interface shows of an arena"""
    s = {"stats": a.stats(), "results": a.results(), "counters": counters(a)}
    for g in range(a.n_games):
        board, st = a.game(g)
        s["game", g] = (board.tobytes(), tuple(sorted(st.items())), a.history(g).tobytes())
        for agent in (0, 1):
            s["tree", g, agent] = (a.tree_nodes(g, agent),) + tuple(bits(x).tobytes() for x in a.root_children(g, agent))
    planes, policy, value, game = a.examples()
    order = np.argsort(game, kind="stable")   # per game, in the order recorded
    s["examples"] = tuple(bits(x[order]).tobytes() for x in (planes, policy, value, game))
    return s


def assert_equal(a, b, what):
    sa, sb = snapshot(a), snapshot(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert sa[k] == sb[k], "%s: %r differs" % (what, k)


def tree_words(path, G, stride):
    """n_nodes[T], cur_pool[T] and the offset of the first node run of a checkpoint, from the documented layout (arena_ckpt.hpp)"""
    per_game = CELLS_PAD + RING * CELLS_PAD + 8 * 4 + 3 * 4 + 2 * 2 * stride + 2 * 4 + 8 + 2 * 4
    raw = open(path, "rb").read()
    off, T = 8 + 28 + 40 + 20 + 32 + G * per_game, 2 * G
    words = np.frombuffer(raw, np.int32, 8 * T, off).reshape(8, T)          # n_nodes, cur_pool, has_root, has_prev, prev_ply, stalled, overflow, pc_n
    node0 = off + 8 * T * 4 + T * CELLS_PAD + T * 8 + 6 * int(words[7].sum()) + 8
    assert struct.unpack_from("<Q", raw, node0 - 8)[0] == int(words[0].sum())
    return words[0], words[1], node0


def continuation(ctx, tmp_path, conf, N, mk_s=None, mk_l=None, on_first=None, **kw):
    """U plays 2N moves; S plays N, saves, is destroyed; L (another seed) loads and plays N: L equals U after each.  Returns the file."""
    path = str(tmp_path / "arena.ckpt")
    u = make(ctx, conf, 11, **kw)
    s = (mk_s or (lambda: make(ctx, conf, 11, **kw)))()
    for _ in range(N):
        move(u)
        move(s)
    assert_equal(s, u, "before the save")
    s.save(path)
    s.close()
    l_ = (mk_l or (lambda: make(ctx, conf, 977, **kw)))()
    l_.load(path)
    assert_equal(l_, u, "after the load")
    for i in range(N):
        move(u)
        move(l_)
        assert_equal(l_, u, "move %d after the load" % (i + 1))
        if i == 0 and on_first:
            on_first(l_)
    u.close()
    return path, l_


def test_continuous_selfplay_c4_with_restarts_labels_and_counters(ctx, tmp_path):
    """agz_arena_selfplay with restart on: games have ended, been labelled and restarted (colours drawn from rng_game) before the save"""
    path = str(tmp_path / "c4.ckpt")
    u, s = make(ctx, C4, 5), make(ctx, C4, 5)
    u.selfplay(14)                                        # uninterrupted
    s.selfplay(6)
    st = s.stats()
    assert 6 <= st["games_finished"] < 14 and st["n_active"] == 8, st      # finished games restarted; labelled and unlabelled rows both present
    v = s.examples()[2]
    assert st["examples"] == v.size > 0
    s.save(path)
    s.close()
    l_ = make(ctx, C4, 4242)
    l_.load(path)
    assert l_.stats() == st
    l_.selfplay(14)
    assert_equal(l_, u, "selfplay continued from the checkpoint")
    assert l_.stats()["games_finished"] >= 14
    rows = []
    for a in (l_, u):                                     # the harvest takes equal rows (finished games only), and leaves equal rows behind
        ex = A.Examples(ctx, 2, 6, 7, 8)
        ex.append_arena(a)
        p, q, v = ex.get()
        rows.append(sorted(bits(p[i]).tobytes() + bits(q[i]).tobytes() + bits(v[i:i + 1]).tobytes() for i in range(len(v))))
        ex.close()
    assert rows[0] == rows[1] and len(rows[0]) > 0
    assert_equal(l_, u, "after the harvest")
    l_.close()
    u.close()


def test_wq9_ring_wrapped_both_pools_trees_across_chunks(ctx, tmp_path):
    """9 moves: the 8-deep ring has wrapped; 2 KB of staging: ~100 nodes a chunk, every tree spans many; both pools hold live trees"""
    kept = []

    def on_first(l_):
        for g in range(l_.n_games):
            for agent in (0, 1):
                vis = l_.root_children(g, agent)[1]
                kept.append(int(vis.sum()) - vis.size)    # visits below the root beyond the 1 every child is created with

    path, l_ = continuation(ctx, tmp_path, WQ9, 9, staging=2048, on_first=on_first)
    n_nodes, cur_pool, _ = tree_words(path, 6, 2 * 81 + 4)
    assert n_nodes.max() > 10 * (2048 // 20), n_nodes     # trees much larger than a chunk
    assert set(cur_pool[n_nodes > 0].tolist()) == {0, 1}, cur_pool
    # a fresh root ends its search with 1 (created) + 1 (prepareRoot) + Budget visits and exactly Budget visits below it; more below the
    # root than this move's simulations (root visits >= Budget + 3 > Budget + 1) is a re-rooted subtree that came through the file
    assert max(kept) > WQ9["Budget"], kept
    l_.close()


@pytest.mark.parametrize("games", [2, 3])
def test_the_smallest_staging_c4(ctx, tmp_path, games):
    """64 bytes of staging, the floor: three nodes a chunk and 64-byte steps through the examples, so every tree is cut, chunks begin and
    end at odd nodes of a tree (the 16-bit runs at odd elements), and a tree's last chunk is shorter than the others"""
    conf = dict(C4, n_games=games, Budget=8)
    path = str(tmp_path / "floor.ckpt")
    u, s = make(ctx, conf, 11), make(ctx, conf, 11, staging=64)
    for _ in range(3):
        move(u)
        move(s)
    n_nodes = [s.tree_nodes(g, agent) for g in range(games) for agent in (0, 1)]
    assert min(n_nodes) > 3 and sum(n_nodes) < 2000 and any(n % 3 for n in n_nodes), n_nodes
    s.save(path)
    assert_equal(s, u, "after the save")
    s.close()
    l_ = make(ctx, conf, 977, staging=64)
    l_.load(path)
    assert_equal(l_, u, "after the load")
    move(u)
    move(l_)
    assert_equal(l_, u, "a move after the load")
    l_.close()
    u.close()


def test_lane_rounds_komi5(ctx, tmp_path):
    """set_parallel(4): rounds of four lanes with virtual loss; the flags are not in the file (all clear at a move boundary)"""
    _, l_ = continuation(ctx, tmp_path, KOMI5, 4, lanes=4)
    l_.close()


def test_capacity_independence_growth_and_a_pool_too_small(ctx, tmp_path):
    big, other = 40000, 61234
    path, l_ = continuation(ctx, tmp_path, KOMI5, 3, mk_s=lambda: make(ctx, KOMI5, 11, max_nodes=big), mk_l=lambda: make(ctx, KOMI5, 977, max_nodes=other),
                            max_nodes=big)
    assert l_.pool_capacity() == (other, 0)
    l_.close()
    # the same file into a tiny AGZ_POOL_GROW arena: the pools grow at the load, the continuation is the uninterrupted one
    u = make(ctx, KOMI5, 11, max_nodes=big)
    for _ in range(3):
        move(u)
    grow = make(ctx, KOMI5, 3, max_nodes=64, policy=capi.POOL_GROW)
    assert grow.pool_capacity() == (64, 0)
    grow.load(path)
    cap, grows = grow.pool_capacity()
    assert grows >= 1 and cap > 64, (cap, grows)
    for i in range(3):
        move(u)
        move(grow)
        assert_equal(grow, u, "grown arena, move %d" % (i + 1))
    grow.close()
    u.close()
    # a strict arena smaller than the fullest tree: AGZ_E_NOMEM, and it plays on as if nothing had been asked
    n_nodes, _, _ = tree_words(path, 4, 2 * 25 + 4)
    small = int(n_nodes.max()) - 1
    tiny, twin = make(ctx, KOMI5, 21, max_nodes=small, Budget=32), make(ctx, KOMI5, 21, max_nodes=small, Budget=32)
    assert capi.lib().agz_arena_load(tiny.h, os.fsencode(path)) == E_NOMEM
    assert b"nodes" in capi.lib().agz_last_error()
    assert tiny.pool_capacity() == (small, 0)
    for a in (tiny, twin):                                 # (one move: the small pools hold a first search)
        a.begin_move()
        a.simulate(8)
        a.end_move(True)
    assert_equal(tiny, twin, "after the refused load")
    tiny.close()
    twin.close()


def test_network_in_the_loop_wq7(ctx, tmp_path):
    """AGZ_INF_NET: the net is saved with agz_net_save and loaded into a second net object for arena L — reattaching it is all a resume needs"""
    def net():
        return A.Net(ctx, 32, 2, 64, 7, 7, 18, 50, bn_mode=capi.BN_IDENTITY)
    n1 = net()
    n1.init_random(99)
    n1.commit()
    n1.save(str(tmp_path / "net.agz"))
    n2 = net()
    n2.load(str(tmp_path / "net.agz"))
    _, l_ = continuation(ctx, tmp_path, WQ7, 3, mk_l=lambda: make(ctx, WQ7, 977, inf=capi.INF_NET, net=n2), inf=capi.INF_NET, net=n1)
    l_.close()
    n1.close()
    n2.close()


def test_save_is_a_no_op_on_the_arena(ctx, tmp_path):
    u, s = make(ctx, KOMI5, 8), make(ctx, KOMI5, 8, staging=512)
    for i in range(4):
        move(u)
        move(s)
        s.save(str(tmp_path / ("s%d.ckpt" % (i % 2))))
        assert_equal(s, u, "after save %d" % i)
    u.close()
    s.close()


def test_refusals_leave_the_arena_and_the_previous_file_alone(ctx, tmp_path):
    L = capi.lib()
    good = str(tmp_path / "good.ckpt")
    a, twin = make(ctx, KOMI5, 8), make(ctx, KOMI5, 8)
    for _ in range(3):
        move(a)
        move(twin)
    a.save(good)
    raw = open(good, "rb").read()
    # save inside a move
    a.begin_move()
    assert L.agz_arena_save(a.h, os.fsencode(str(tmp_path / "mid.ckpt"))) == E_STATE
    assert L.agz_arena_load(a.h, os.fsencode(good)) == E_STATE
    assert not os.path.exists(tmp_path / "mid.ckpt") and not os.path.exists(tmp_path / "mid.ckpt.tmp")
    a.simulate(KOMI5["Budget"])
    a.end_move(True)
    move(twin)
    assert_equal(a, twin, "after a save refused inside a move")
    # another configuration: the field is named
    for over, field in ((dict(n_games=5), b"n_games"), (dict(m=6, n=6), b"game.m"), (dict(kind=capi.GAME_MNK), b"game.kind"), (dict(Budget=33), b"mcts.Budget")):
        o = make(ctx, KOMI5, 8, **over)
        assert L.agz_arena_load(o.h, os.fsencode(good)) == E_INVALID, over
        assert field in L.agz_last_error(), (over, L.agz_last_error())
        o.close()
    # files cut inside the header, the per-game state, the nodes, the examples and the end section; one kids_off past n_nodes; a missing path
    G, stride = 4, 2 * 25 + 4
    n_nodes, _, node0 = tree_words(good, G, stride)
    N = int(n_nodes.sum())
    ex0 = node0 + 20 * N + 16 * 8 + 8
    assert ex0 < len(raw) - 16
    bad = str(tmp_path / "bad.ckpt")
    for cut in (60, 128 + 5000, node0 + 10 * N, ex0 + (len(raw) - 16 - ex0) // 2, len(raw) - 7):
        open(bad, "wb").write(raw[:cut])
        assert L.agz_arena_load(a.h, os.fsencode(bad)) == E_INVALID, cut
        assert b"truncated" in L.agz_last_error(), (cut, L.agz_last_error())
    first = int(np.flatnonzero(n_nodes > 1)[0])
    koff = node0 + 12 * N + 4 * int(n_nodes[:first].sum())   # kids_off of that tree's root
    assert struct.unpack_from("<i", raw, koff)[0] == 1
    open(bad, "wb").write(raw[:koff] + struct.pack("<i", int(n_nodes[first])) + raw[koff + 4:])
    assert L.agz_arena_load(a.h, os.fsencode(bad)) == E_INVALID
    assert b"kids_off" in L.agz_last_error(), L.agz_last_error()
    assert L.agz_arena_load(a.h, os.fsencode(str(tmp_path / "nothing.ckpt"))) == E_INVALID
    assert b"cannot open" in L.agz_last_error()
    move(a)
    move(twin)
    assert_equal(a, twin, "after the refused loads")
    # a save that cannot create its file: the directory is read-only (where that does not bind this user, the temporary's name is taken by a
    # directory); the previous good file is untouched and nothing is left behind
    ro = tmp_path / "ro"
    ro.mkdir()
    kept = str(ro / "kept.ckpt")
    a.save(kept)
    before = open(kept, "rb").read()
    os.chmod(ro, 0o555)
    still_writable = os.access(ro, os.W_OK)
    if still_writable:
        os.chmod(ro, 0o755)
        os.mkdir(kept + ".tmp")
    move(a)
    move(twin)
    try:
        assert L.agz_arena_save(a.h, os.fsencode(kept)) == E_INVALID
        assert b"cannot open" in L.agz_last_error()
    finally:
        os.chmod(ro, 0o755)
    assert open(kept, "rb").read() == before
    assert sorted(os.listdir(ro)) == (["kept.ckpt", "kept.ckpt.tmp"] if still_writable else ["kept.ckpt"])
    assert_equal(a, twin, "after the refused save")
    # and the good file still loads: a goes back three moves, twin-of-then continues equal
    a.load(good)
    fresh = make(ctx, KOMI5, 1)
    fresh.load(good)
    move(a)
    move(fresh)
    assert_equal(a, fresh, "both loaded from the good file")
    for x in (a, twin, fresh):
        x.close()
