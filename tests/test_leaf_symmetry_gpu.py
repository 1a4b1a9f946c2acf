"""GPU: leaf evaluation under a board symmetry (agz_arena_set_leaf_symmetry / agz_mcts_set_leaf_symmetry).

With the setting on, k_select / k_leaf write a network agent's input through S_k and k_expand / k_expand_prep read the policy row back
through dst_k.  The reference for all of it is a HOST inferencer that does the same thing in numpy on an arena with the setting OFF:
it is handed the untransformed encoder planes and the board (AGZ_INF_CALLBACK), works out k from the board (a Python restatement of
mix32 — tests/test_sym_cpu.py ties it to agz_leaf_symmetry_of), turns the planes with np.rot90 / .T, calls the same HIP network and
turns the policy back.  Roots (children, visits, blackScores bits, prior bits), histories, counters and the recorded examples are
compared bit for bit after every ply.  Nothing here depends on timing."""
import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -6
STAT_KEYS = ("sims_total", "sims_nonnull", "nn_evals", "moves_played", "games_finished", "examples", "tree_full")
SEED = 0x9E3779B97F4A7C15


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def leaf_k(seed, board, to_move):
    """AGZ_SYM_RANDOM's k, restated (include/agz.h)"""
    with np.errstate(over="ignore"):
        b = np.asarray(board, np.uint32).reshape(-1)
        ph = mix32(np.arange(b.size, dtype=np.uint32) * np.uint32(4) + b + np.uint32(1)).sum(dtype=np.uint32)
        ph = np.uint32(ph + mix32(np.uint32(0xABCD0000) + np.uint32(to_move)))
        fold = np.uint32(seed & 0xFFFFFFFF) ^ np.uint32((seed >> 32) & 0xFFFFFFFF)
        return int(mix32(ph ^ fold) >> np.uint32(29))


def S_apply(x, k):
    """S_k = R^(k&3) o T^(k>>2) on the last two axes; (R x)[i][j] = x[j][m-1-i] is np.rot90's own quarter turn"""
    y = np.swapaxes(x, -1, -2) if k >> 2 else x
    return np.rot90(y, k & 3, axes=(-2, -1))


def S_inverse(x, k):
    """(R^r o T^t)^-1 = T^t o R^-r"""
    y = np.rot90(x, -(k & 3), axes=(-2, -1))
    return np.swapaxes(y, -1, -2) if k >> 2 else y


def sym_nn(net, S, mode, seed, seen):
    """the host side of symmetric evaluation: planes through S_k, the network, the policy's board part back through S_k^-1"""
    def f(leaves):
        x = np.ascontiguousarray(leaves["planes"])
        n = x.shape[0]
        ks = [leaf_k(seed, leaves["board"][i], leaves["to_move"][i]) if mode == capi.SYM_RANDOM else mode - capi.SYM_FIXED for i in range(n)]
        seen.update(ks)
        xs = np.stack([S_apply(x[i], ks[i]) for i in range(n)])
        p, v = net.infer(np.ascontiguousarray(xs))
        out = p.copy()                                              # the pass entry (last) and anything past the board stay
        for i in range(n):
            out[i, :S * S] = S_inverse(p[i, :S * S].reshape(S, S), ks[i]).reshape(-1)
        return out, v
    return f


def make_net(ctx, S, F, seed=5):
    net = A.Net(ctx, 32, 2, 64, S, S, F, S * S + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(seed)
    net.commit()
    net.set_compute_mode(capi.COMPUTE_F32_MFMA | capi.COMPUTE_FORCE)     # one arithmetic whatever the batch size
    return net


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(a, b, what, examples=True):
    for g in range(a.n_games):
        np.testing.assert_array_equal(a.history(g), b.history(g), err_msg="%s: history of game %d" % (what, g))
        for agent in (0, 1):
            ra, rb = a.root_children(g, agent), b.root_children(g, agent)
            for x, y, name in zip(ra, rb, ("moves", "visits", "blackScores", "priors")):
                np.testing.assert_array_equal(bits(x), bits(y), err_msg="%s: game %d agent %d %s" % (what, g, agent, name))
    if examples:                                                    # per game, in the order recorded (the row order within a move is an atomic's)
        ea, eb = a.examples(), b.examples()
        oa, ob = np.argsort(ea[3], kind="stable"), np.argsort(eb[3], kind="stable")
        for x, y, name in zip(ea, eb, ("planes", "policy", "value", "game")):
            np.testing.assert_array_equal(bits(x[oa]), bits(y[ob]), err_msg="%s: example %s" % (what, name))
    sa, sb = a.stats(), b.stats()
    for key in STAT_KEYS:
        assert sa[key] == sb[key], (what, key, sa[key], sb[key])


def roots_differ(a, b):
    for g in range(a.n_games):
        for agent in (0, 1):
            ra, rb = a.root_children(g, agent), b.root_children(g, agent)
            if any(x.shape != y.shape or not np.array_equal(bits(x), bits(y)) for x, y in zip(ra, rb)):
                return True
    return False


def move(a, record=True):
    a.begin_move()
    a.simulate(a.mconf.Budget)
    a.end_move(record)


GAMES = {
    "komi5": dict(kind=capi.GAME_KOMI, m=5, k=3, komi=0.0, encoder=capi.ENC_TWOPLANE, F=2, most=6),
    "mnk6": dict(kind=capi.GAME_MNK, m=6, k=4, komi=0.0, encoder=capi.ENC_TWOPLANE, F=2, most=8),
    "go9": dict(kind=capi.GAME_WQ, m=9, k=0, komi=5.5, encoder=capi.ENC_WQ, F=18, most=30),
}


def make_arena(ctx, game, G, budget, kinds, net, mode, seen, lanes=1, seed=5, opening_seed=9, least=0):
    """kinds[agent] is 'net' (the device network) or 'cb' (the host function doing the symmetry itself).  `mode` is what the arena is
    set to where it has a network agent and what the callback applies; an arena of callbacks alone stays OFF."""
    c = GAMES[game]
    S = c["m"]
    dev = A.Arena(ctx, c["kind"], S, S, c["k"], c["komi"], encoder=c["encoder"], n_games=G, seed=seed, Budget=budget)
    if lanes > 1:
        dev.set_parallel(lanes)
    for agent, kind in enumerate(kinds):
        if kind == "net":
            dev.set_inferencer(agent, capi.INF_NET, net)
        else:
            dev.set_inferencer_callback(agent, sym_nn(net, S, mode, SEED, seen), S * S + 1)
    if "net" in kinds and mode != capi.SYM_OFF:
        dev.set_leaf_symmetry(mode, SEED)
    dev.reset()
    dev.random_moves(np.random.default_rng(opening_seed).integers(least, c["most"], size=G).astype(np.int32), opening_seed)
    return dev


def test_random_symmetry_equals_a_host_inferencer_that_does_the_same(ctx):
    """The main parity test: 9x9 Go with the WQ encoder (history planes go through the map too).  X: both agents the device network,
    AGZ_SYM_RANDOM.  Y: both agents the host function, symmetry OFF.  Z: agent 0 the device network, agent 1 the host function,
    AGZ_SYM_RANDOM (a callback agent's planes stay untransformed).  W: X with the symmetry OFF — it must differ, or nothing was tested."""
    G, budget = 12, 32
    net = make_net(ctx, 9, 18)
    seen_y, seen_z = set(), set()
    x = make_arena(ctx, "go9", G, budget, ("net", "net"), net, capi.SYM_RANDOM, None, least=4)
    y = make_arena(ctx, "go9", G, budget, ("cb", "cb"), net, capi.SYM_RANDOM, seen_y, least=4)
    z = make_arena(ctx, "go9", G, budget, ("net", "cb"), net, capi.SYM_RANDOM, seen_z, least=4)
    w = make_arena(ctx, "go9", G, budget, ("net", "net"), net, capi.SYM_OFF, None, least=4)
    differs = False
    for ply in range(4):
        for dev in (x, y, z, w):
            move(dev)
        assert_same(y, x, "host vs device, ply %d" % ply)
        assert_same(z, x, "mixed vs device, ply %d" % ply)
        differs = differs or roots_differ(w, x)
    assert seen_y == set(range(8)), seen_y                          # the callback saw every one of the eight maps
    assert seen_z, seen_z
    assert differs, "symmetry OFF gave the same roots as AGZ_SYM_RANDOM: the network is equivariant or the setting did nothing"
    for dev in (x, y, z, w):
        dev.close()
    net.close()


@pytest.mark.parametrize("k", [1, 4, 6])
@pytest.mark.parametrize("game", ["komi5", "mnk6"])
def test_fixed_symmetry_on_an_odd_and_an_even_board(ctx, game, k):
    """AGZ_SYM_FIXED + k: k = 1 is no involution (a wrong inverse shows), 4 is the transpose, 6 a reflection; the even board catches an
    m-1-i slip an odd one can hide"""
    G, budget = 6, 24
    net = make_net(ctx, GAMES[game]["m"], 2, seed=11 + k)
    seen = set()
    x = make_arena(ctx, game, G, budget, ("net", "net"), net, capi.SYM_FIXED + k, None)
    y = make_arena(ctx, game, G, budget, ("cb", "cb"), net, capi.SYM_FIXED + k, seen)
    w = make_arena(ctx, game, G, budget, ("net", "net"), net, capi.SYM_OFF, None)
    differs = False
    for ply in range(3):
        for dev in (x, y, w):
            move(dev)
        assert_same(y, x, "%s k %d ply %d" % (game, k, ply))
        differs = differs or roots_differ(w, x)
    assert seen == {k} and differs
    for dev in (x, y, w):
        dev.close()
    net.close()


def test_lane_rounds_go_through_k_leaf_and_k_expand_prep(ctx):
    """set_parallel(4): the leaf work runs in k_leaf, the expansion list in k_expand_prep; a fixed k and the per-position one"""
    G, budget = 6, 32
    net = make_net(ctx, 9, 18)
    for mode in (capi.SYM_FIXED + 1, capi.SYM_RANDOM):
        seen = set()
        x = make_arena(ctx, "go9", G, budget, ("net", "net"), net, mode, None, lanes=4, least=4)
        y = make_arena(ctx, "go9", G, budget, ("cb", "net"), net, mode, seen, lanes=4, least=4)
        yy = make_arena(ctx, "go9", G, budget, ("cb", "cb"), net, mode, seen, lanes=4, least=4)
        for ply in range(3):
            for dev in (x, y, yy):
                move(dev)
            assert_same(y, x, "lanes, mode %d, mixed, ply %d" % (mode, ply))
            assert_same(yy, x, "lanes, mode %d, host, ply %d" % (mode, ply))
        assert len(seen) >= (1 if mode != capi.SYM_RANDOM else 4), seen
        for dev in (x, y, yy):
            dev.close()
    net.close()


class Host:
    """the caller's game of a single tree (as tests/test_callback_inferencer_gpu.py)"""

    def __init__(self, okind, m, n, k, komi):
        self.g = O.Game(okind, m, n, k, komi)
        self.g.set_to_move(O.BLACK)
        self.moves, self.boards = [], []

    def apply(self, player, mv):
        self.g.apply(player, mv)
        self.moves.append(mv)
        self.boards.append(self.g.board())
        self.g.set_to_move(O.WHITE if player == O.BLACK else O.BLACK)

    def state_kw(self):
        n = len(self.moves)
        return dict(board=self.g.board(), to_move=self.g.to_move(), n_moves=n, passes=max(self.g.passes(), 0), hash=self.g.hash(),
                    last_moves=self.moves, historical=np.array(self.boards[max(0, n - 8):], np.int32))


@pytest.mark.parametrize("mode", [capi.SYM_FIXED + 6, capi.SYM_RANDOM], ids=["fixed6", "random"])
def test_a_single_tree_and_its_re_rooted_successors(ctx, mode):
    """agz_mcts_set_leaf_symmetry: one tree searched for both colours in turn (every search after the first runs on the re-rooted tree)"""
    S, budget = 6, 48
    net = make_net(ctx, S, 2, seed=3)
    seen = set()
    dev = A.Mcts(ctx, capi.GAME_MNK, S, S, 4, Budget=budget)
    dev.set_inferencer(capi.INF_NET, net)
    dev.set_leaf_symmetry(mode, SEED)
    cb = A.Mcts(ctx, capi.GAME_MNK, S, S, 4, Budget=budget)
    cb.set_inferencer_callback(sym_nn(net, S, mode, SEED, seen), S * S + 1)
    off = A.Mcts(ctx, capi.GAME_MNK, S, S, 4, Budget=budget)
    off.set_inferencer(capi.INF_NET, net)
    host = Host(O.MNK, S, S, 4, 0.0)
    player, differs = O.BLACK, False
    for turn in range(3):
        for t in (dev, cb, off):
            t.set_game(**host.state_kw())
        b1, b2, _ = dev.search(player), cb.search(player), off.search(player)
        assert b1 == b2, turn
        for x, y, z in zip(dev.root_children(), cb.root_children(), off.root_children()):
            np.testing.assert_array_equal(bits(x), bits(y), err_msg="turn %d" % turn)
            differs = differs or x.shape != z.shape or not np.array_equal(bits(x), bits(z))
        assert dev.nodes() == cb.nodes()
        host.apply(player, b1)
        player = O.WHITE if player == O.BLACK else O.BLACK
    assert differs and seen
    for t in (dev, cb, off):
        t.close()
    net.close()


def test_split_step_with_random_symmetry(ctx):
    """416 games of 9x9 in the measured mode (Winograd fp16x2, K = 256, two tower queues): the split step's two half-arena pipelines
    against the joined step, AGZ_SYM_RANDOM on both; agz_arena_split_steps says the split step was really taken"""
    S, G, budget = 9, 416, 8
    net = A.Net(ctx, 256, 4, 64, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(1337)
    net.commit()
    net.set_compute_mode(capi.COMPUTE_WINO_H2)
    net.set_tower_queues(2)
    arenas = []
    for split in (0, 1):
        dev = A.Arena(ctx, capi.GAME_WQ, S, S, 0, 7.5, encoder=capi.ENC_WQ, n_games=G, seed=31, Budget=budget)
        dev.set_inferencer(0, capi.INF_NET, net)
        dev.set_inferencer(1, capi.INF_NET, net)
        dev.set_leaf_symmetry(capi.SYM_RANDOM, SEED)
        dev.reset(np.array([(i % 2) == 1 for i in range(G)], dtype=np.uint8))
        dev.random_moves(np.random.default_rng(31).integers(0, 30, size=G).astype(np.int32), 31)
        dev.set_split(split)
        arenas.append(dev)
    for mv in range(2):
        for dev in arenas:
            move(dev)
        assert_same(arenas[1], arenas[0], "split vs joined, move %d" % mv)
    joined, split = arenas[0].split_steps(), arenas[1].split_steps()
    assert joined[0] == 0 and joined[1] == 2 * budget, joined
    assert split[0] == 2 * budget and split[1] == 0, split
    for dev in arenas:
        dev.close()
    net.close()


def test_checkpoint_continues_bit_for_bit_once_the_setting_is_re_applied(ctx, tmp_path):
    """the setting is not in the file (AGZARN01 unchanged): save between two moves with the symmetry on, load into a fresh arena,
    re-apply it — the continuation equals the uninterrupted arena; without re-applying it, it does not"""
    G, budget = 6, 32
    net = make_net(ctx, 9, 18)
    path = str(tmp_path / "sym.ckpt")
    u = make_arena(ctx, "go9", G, budget, ("net", "net"), net, capi.SYM_RANDOM, None, least=4)
    s = make_arena(ctx, "go9", G, budget, ("net", "net"), net, capi.SYM_RANDOM, None, least=4)
    for dev in (u, s):
        move(dev)
    s.save(path)
    s.close()
    loaded = []
    for mode in (capi.SYM_RANDOM, capi.SYM_OFF):
        c = GAMES["go9"]
        l_ = A.Arena(ctx, c["kind"], 9, 9, c["k"], c["komi"], encoder=c["encoder"], n_games=G, seed=977, Budget=budget)
        for agent in (0, 1):
            l_.set_inferencer(agent, capi.INF_NET, net)
        l_.load(path)
        l_.set_leaf_symmetry(mode, SEED)
        loaded.append(l_)
    assert_same(loaded[0], u, "after the load")
    differs = False
    for i in range(2):
        for dev in [u] + loaded:
            move(dev)
        assert_same(loaded[0], u, "move %d after the load" % (i + 1))
        differs = differs or roots_differ(loaded[1], u)
    assert differs
    for dev in [u] + loaded:
        dev.close()
    net.close()


def test_argument_checks_and_off_after_on(ctx):
    L = capi.lib()
    c4 = A.Arena(ctx, capi.GAME_C4, 6, 7, 4, n_games=2, Budget=4)
    assert L.agz_arena_set_leaf_symmetry(c4.h, capi.SYM_RANDOM, 1) == E_UNSUPPORTED
    assert L.agz_arena_set_leaf_symmetry(c4.h, capi.SYM_OFF, 1) == E_UNSUPPORTED
    c4.close()
    rect = A.Arena(ctx, capi.GAME_MNK, 3, 4, 3, n_games=2, Budget=4)
    assert L.agz_arena_set_leaf_symmetry(rect.h, capi.SYM_FIXED + 2, 1) == E_UNSUPPORTED
    with pytest.raises(A.AgzError, match="agz_arena_set_leaf_symmetry"):
        rect.set_leaf_symmetry(capi.SYM_RANDOM, 1)
    rect.close()
    tree = A.Mcts(ctx, capi.GAME_C4, 6, 7, 4, Budget=4)
    assert L.agz_mcts_set_leaf_symmetry(tree.h, capi.SYM_RANDOM, 1) == E_UNSUPPORTED
    assert L.agz_mcts_set_leaf_symmetry(None, capi.SYM_RANDOM, 1) == E_INVALID
    tree.close()
    assert L.agz_arena_set_leaf_symmetry(None, capi.SYM_RANDOM, 1) == E_INVALID

    G, budget = 4, 16
    net = make_net(ctx, 5, 2)
    a = make_arena(ctx, "komi5", G, budget, ("net", "net"), net, capi.SYM_OFF, None)
    for bad in (-1, 2, 7, 16, 100):
        assert L.agz_arena_set_leaf_symmetry(a.h, bad, 1) == E_INVALID, bad
    a.begin_move()
    assert L.agz_arena_set_leaf_symmetry(a.h, capi.SYM_RANDOM, 1) == E_STATE      # inside a move
    a.simulate(budget)
    a.end_move(True)
    # OFF after ON gives back the OFF trees: b never had the setting, a has it switched on for one move and off again
    b = make_arena(ctx, "komi5", G, budget, ("net", "net"), net, capi.SYM_OFF, None)
    move(b)
    assert_same(a, b, "both OFF")
    a.set_leaf_symmetry(capi.SYM_FIXED + 3, 7)
    a.set_leaf_symmetry(capi.SYM_OFF)
    for dev in (a, b):
        move(dev)
    assert_same(a, b, "OFF after ON")
    a.set_leaf_symmetry(capi.SYM_FIXED + 0, 7)                                   # S_0 is the identity: the ON path with k = 0 changes nothing
    for dev in (a, b):
        move(dev)
    assert_same(a, b, "FIXED + 0")
    a.set_leaf_symmetry(capi.SYM_FIXED + 3, 7)
    for dev in (a, b):
        move(dev)
    assert roots_differ(a, b)
    a.close()
    b.close()
    net.close()
