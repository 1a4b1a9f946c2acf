"""GPU: the split simulation step (agz_arena_set_split, agz_debug.h) against the joined step.

Where one shared net runs the chained Winograd fp16x2 tower of the arena's batch as two half-batch chains, agz_arena_simulate enqueues
the two halves of the arena as pipelines of their own on the context's two queues, with no event between them and a lazy join.  Every
test here runs two arenas on the same seed, net and openings — set_split(0) and set_split(1 | 2) — and compares them BIT FOR BIT after
every move: boards, game state, histories, both agents' root children (moves, visits, blackScores bits, prior bits), examples and the
statistics.  agz_arena_split_steps says which path the steps really took.  Nothing here depends on timing.
"""
import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi

pytestmark = pytest.mark.gpu

# the small shape: 9x9 Go, K = 256, four blocks, two tower queues.  416 games: a half of 208 boards still fills the chip with 128-row tiles
# of the input convolution (agz_net::fwd_plan), so the half runs the kernels of the whole batch — the split path's condition
SMALL_S, SMALL_G = 9, 416

STAT_KEYS = ("sims_total", "sims_nonnull", "nn_evals", "moves_played", "games_finished", "examples", "tree_full", "path_nodes", "children_read")


def make_net(ctx, S, K, L, seed=1337, queues=2):
    net = A.Net(ctx, K, L, 64, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(seed)
    for i in range(net.num_params()):
        name, n = net.param_info(i)
        if name.endswith("_gamma"):
            net.set_param(i, np.ones(n, np.float32))
        elif name.endswith("_beta"):
            net.set_param(i, np.zeros(n, np.float32))
    net.commit()
    net.set_compute_mode(capi.COMPUTE_WINO_H2)
    net.set_tower_queues(queues)
    return net


def make_arena(ctx, S, G, budget, seed, nets, mode, most, lanes=1, callback=None, max_nodes=0):
    dev = A.Arena(ctx, capi.GAME_WQ, S, S, 0, 7.5, encoder=capi.ENC_WQ, n_games=G, seed=seed, Budget=budget, max_nodes=max_nodes)
    if lanes > 1:
        dev.set_parallel(lanes)
    dev.set_inferencer(0, capi.INF_NET, nets[0])
    if callback is not None:
        dev.set_inferencer_callback(1, callback, S * S + 1)
    else:
        dev.set_inferencer(1, capi.INF_NET, nets[-1])
    dev.reset(np.array([(i % 2) == 1 for i in range(G)], dtype=np.uint8))
    dev.random_moves(np.random.default_rng(seed).integers(0, most, size=G).astype(np.int32), seed)
    dev.set_split(mode)
    return dev


def assert_same(a, b, G, games, what):
    for g in games:
        (ba, sa), (bb, sb) = a.game(g), b.game(g)
        np.testing.assert_array_equal(ba, bb, err_msg="%s: board of game %d" % (what, g))
        assert sa == sb, (what, g, sa, sb)
        np.testing.assert_array_equal(a.history(g), b.history(g), err_msg="%s: history of game %d" % (what, g))
        for agent in (0, 1):
            ra, rb = a.root_children(g, agent), b.root_children(g, agent)
            np.testing.assert_array_equal(ra[0], rb[0], err_msg="%s: game %d agent %d moves" % (what, g, agent))
            np.testing.assert_array_equal(ra[1], rb[1], err_msg="%s: game %d agent %d visits" % (what, g, agent))
            np.testing.assert_array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32), err_msg="%s: game %d agent %d blackScores" % (what, g, agent))
            np.testing.assert_array_equal(ra[3].view(np.uint32), rb[3].view(np.uint32), err_msg="%s: game %d agent %d priors" % (what, g, agent))
    # (k_end_move hands out example rows through an atomic counter: the row order among the games of one move is the launch's, so compare
    #  per game — a stable sort by game keeps each game's examples in the order they were recorded)
    ea, eb = a.examples(), b.examples()
    oa, ob = np.argsort(ea[3], kind="stable"), np.argsort(eb[3], kind="stable")
    for x, y, name in zip(ea, eb, ("planes", "policy", "value", "game")):
        x, y = x[oa], y[ob]
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y,
                                      err_msg="%s: example %s" % (what, name))
    s1, s0 = a.stats(), b.stats()
    for k in STAT_KEYS:
        if k in s1:
            assert s1[k] == s0[k], (what, k, s1[k], s0[k])


def run_pair(ctx, S, G, budget, moves, nets, mode, most, games, lanes=1, callback=None, simulate_in=None, max_nodes=0):
    """two arenas, joined (0) and `mode`; returns their split_steps() after `moves` whole moves compared bit for bit"""
    arenas = [make_arena(ctx, S, G, budget, 31, nets, m, most, lanes, callback, max_nodes) for m in (0, mode)]
    for mv in range(moves):
        for dev in arenas:
            dev.begin_move()
        if simulate_in is None:
            for dev in arenas:
                dev.simulate(budget)
        else:                                   # the two arenas' steps interleaved on ONE context (one's halves in flight under the other's)
            done = 0
            while done < budget:
                k = min(simulate_in, budget - done)
                for dev in arenas:
                    dev.simulate(k)
                done += k
        for dev in arenas:
            dev.end_move(True)
        assert_same(arenas[1], arenas[0], G, games, "move %d" % mv)
    steps = [dev.split_steps() for dev in arenas]
    for dev in arenas:
        dev.close()
    return steps


@pytest.mark.parametrize("mode", [1, 2])
def test_split_step_at_the_headline_shape(ctx, mode):
    """512 games, 19x19, K=256, L=20 (what bench.py times), a short Budget, three whole moves: the third re-roots real trees."""
    S, G, budget = 19, 512, 10
    net = make_net(ctx, S, 256, 20, queues=0)       # the library default: two queues from 256 boards
    games = list(range(0, G, 23)) + [G // 2 - 1, G // 2, G - 1]
    joined, split = run_pair(ctx, S, G, budget, 3, [net], mode, 200, games, max_nodes=20000)
    assert joined[0] == 0 and joined[1] == 3 * budget, joined
    assert split[0] == 3 * budget and split[1] == 0 and split[2], split
    net.close()


@pytest.mark.parametrize("mode,simulate_in", [(1, None), (2, None), (1, 1), (1, 3)])
def test_split_step_small_shape(ctx, mode, simulate_in):
    """416 games of 9x9 Go on a K=256, 4-block net with two tower queues: small, and still the chained tower in two chunks of 208 boards.
    Every game compared; with simulate_in the two arenas' steps alternate on the one context."""
    S, G, budget = SMALL_S, SMALL_G, 40
    assert capi.wino_h2_chained(S, S, 256) == 1
    net = make_net(ctx, S, 256, 4)
    joined, split = run_pair(ctx, S, G, budget, 4, [net], mode, 30, range(G), simulate_in=simulate_in)
    assert joined[0] == 0, joined
    assert split[0] == 4 * budget and split[1] == 0, split
    net.close()


@pytest.mark.parametrize("case", ["lanes", "two_nets", "callback", "one_queue", "odd_half"])
def test_every_other_case_takes_the_joined_step(ctx, case):
    """lane rounds, two different nets, a callback inferencer, a one-queue tower, a half that is no multiple of four boards: set_split(1)
    changes nothing — identical results and not one step on the split path."""
    S, G, budget = SMALL_S, SMALL_G, 24
    nets = [make_net(ctx, S, 256, 4, queues=1 if case == "one_queue" else 2)]
    kw = {}
    if case == "lanes":
        kw["lanes"] = 2
    if case == "two_nets":
        nets.append(make_net(ctx, S, 256, 4, seed=7))
    if case == "callback":
        def nn(leaves):
            return nets[0].infer(np.ascontiguousarray(leaves["planes"]))
        kw["callback"] = nn
    if case == "odd_half":
        G = SMALL_G + 2
    joined, split = run_pair(ctx, S, G, budget, 2, nets, 1, 30, range(0, G, 5), **kw)
    assert joined[0] == 0 and split[0] == 0 and not split[2], (joined, split)
    assert split[1] == joined[1] > 0
    for n in nets:
        n.close()


def test_lazy_join_between_single_steps(ctx):
    """simulate(1) interleaved with stats(), root_children(), game(), net.infer() on the same context and ctx.sync(): each of them must see
    everything both queues were given (the join happens there, not at the end of simulate), and the search must go on unharmed."""
    S, G, budget = SMALL_S, SMALL_G, 30
    net = make_net(ctx, S, 256, 4)
    arenas = [make_arena(ctx, S, G, budget, 31, [net], m, 30) for m in (0, 1)]
    planes = np.random.default_rng(3).integers(-1, 2, size=(8, 18, S, S)).astype(np.float32)
    p_ref, v_ref = net.infer(planes)
    for mv in range(2):
        for dev in arenas:
            dev.begin_move()
        for step in range(budget):
            for dev in arenas:
                dev.simulate(1)
            kind = step % 5
            if kind == 0:
                s1, s0 = arenas[1].stats(), arenas[0].stats()
                assert s1["sims_total"] == s0["sims_total"] and s1["nn_evals"] == s0["nn_evals"], (mv, step)
            elif kind == 1:
                for g in (0, G // 2 - 1, G // 2, G - 1):          # both halves
                    agent = 0 if arenas[0].root_children(g, 0)[1].sum() >= arenas[0].root_children(g, 1)[1].sum() else 1
                    ra, rb = arenas[1].root_children(g, agent), arenas[0].root_children(g, agent)
                    np.testing.assert_array_equal(ra[1], rb[1], err_msg="move %d step %d game %d" % (mv, step, g))
                    np.testing.assert_array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32))
            elif kind == 2:
                p, v = net.infer(planes)                           # the net's buffers are the ones the halves run through
                np.testing.assert_array_equal(p.view(np.uint32), p_ref.view(np.uint32))
                np.testing.assert_array_equal(v.view(np.uint32), v_ref.view(np.uint32))
            elif kind == 3:
                ctx.sync()
                assert arenas[1].tree_nodes(G - 1, 0) == arenas[0].tree_nodes(G - 1, 0)
                assert arenas[1].tree_nodes(G - 1, 1) == arenas[0].tree_nodes(G - 1, 1)
        for dev in arenas:
            dev.end_move(True)
        assert_same(arenas[1], arenas[0], G, range(G), "move %d" % mv)
    assert arenas[1].split_steps()[0] == 2 * budget and arenas[0].split_steps()[0] == 0
    for dev in arenas:
        dev.close()
    net.close()
