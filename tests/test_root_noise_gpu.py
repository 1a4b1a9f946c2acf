"""GPU: Dirichlet noise on the root priors (agz_arena_set_root_noise / agz_mcts_set_root_noise, DESIGN.md §2 root-noise).

The reference has no such thing, so the references here are (a) the host function agz_root_noise_of — tests/test_root_noise_cpu.py ties
it bit for bit to a pure-Python restatement of the declared definition — for eta, (b) a TWIN arena from the same seed without noise for
the priors the noise was mixed into, with the mix restated in numpy float32 (one rounding per operation), and (c) twin arenas for
everything that must stay bit-identical: off, the checkpoint continuation, play() against the begin / simulate / end rounds.  Roots
(children, visits, blackScores bits, prior bits), histories, counters and the recorded examples are compared bit for bit.  Nothing here
depends on timing."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
STAT_KEYS = ("sims_total", "sims_nonnull", "nn_evals", "moves_played", "games_finished", "examples", "tree_full")
G = 8

GAMES = {
    "komi5": dict(kind=capi.GAME_KOMI, m=5, n=5, k=3, komi=0.0, encoder=capi.ENC_TWOPLANE, Budget=24, most=6),
    "mnk6": dict(kind=capi.GAME_MNK, m=6, n=6, k=4, komi=0.0, encoder=capi.ENC_TWOPLANE, Budget=16, most=8),
    "go9": dict(kind=capi.GAME_WQ, m=9, n=9, k=0, komi=5.5, encoder=capi.ENC_WQ, Budget=16, most=12),
    "c4": dict(kind=capi.GAME_C4, m=6, n=7, k=4, komi=0.0, encoder=capi.ENC_TWOPLANE, Budget=16, most=0),
}


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def mix(eps, prior, eta):
    """fadd(fmul(1 - eps, prior), fmul(eps, eta)) in float32, one rounding per operation"""
    eps, prior, eta = np.float32(eps), np.asarray(prior, np.float32), np.asarray(eta, np.float32)
    c1 = np.float32(np.float32(1.0) - eps)
    return (c1 * prior).astype(np.float32) + (eps * eta).astype(np.float32)


def make_net(ctx):
    net = A.Net(ctx, 32, 2, 64, 9, 9, 18, 82, bn_mode=capi.BN_IDENTITY)
    net.init_random(5)
    net.commit()
    net.set_compute_mode(capi.COMPUTE_F32_MFMA | capi.COMPUTE_FORCE)     # one arithmetic whatever the batch size
    return net


def make(ctx, game, seed=5, kinds=(capi.INF_HASH, capi.INF_HASH), net=None, noise=None, lanes=1, opening=True, **over):
    """noise: None (never configured) or the keyword arguments of set_root_noise"""
    c = dict(GAMES[game], **over)
    most = c.pop("most")
    a = A.Arena(ctx, c.pop("kind"), c.pop("m"), c.pop("n"), n_games=G, seed=seed, **c)
    if lanes > 1:
        a.set_parallel(lanes)
    for agent in (0, 1):
        a.set_inferencer(agent, kinds[agent], net if kinds[agent] == capi.INF_NET else None)
    if noise is not None:
        a.set_root_noise(**noise)
    a.reset(np.array([g % 2 for g in range(G)], np.uint8))             # both agents get to search first somewhere
    if opening and most:
        a.random_moves(np.random.default_rng(9).integers(0, most, size=G).astype(np.int32), 9)
    return a


def move(a, record=True):
    a.begin_move()
    a.simulate(a.mconf.Budget)
    a.end_move(record)


def assert_same(a, b, what):
    for g in range(a.n_games):
        np.testing.assert_array_equal(a.history(g), b.history(g), err_msg="%s: history of game %d" % (what, g))
        for agent in (0, 1):
            ra, rb = a.root_children(g, agent), b.root_children(g, agent)
            for x, y, name in zip(ra, rb, ("moves", "visits", "blackScores", "priors")):
                np.testing.assert_array_equal(bits(x), bits(y), err_msg="%s: game %d agent %d %s" % (what, g, agent, name))
    ea, eb = a.examples(), b.examples()                                # per game, in the order recorded
    oa, ob = np.argsort(ea[3], kind="stable"), np.argsort(eb[3], kind="stable")
    for x, y, name in zip(ea, eb, ("planes", "policy", "value", "game")):
        np.testing.assert_array_equal(bits(x[oa]), bits(y[ob]), err_msg="%s: example %s" % (what, name))
    sa, sb = a.stats(), b.stats()
    for key in STAT_KEYS:
        assert sa[key] == sb[key], (what, key, sa[key], sb[key])


def searching_agent(a, g):
    _, st = a.game(g)
    if st["ended"]:
        return None
    return 0 if (st["to_move"] == capi.BLACK) == bool(st["a_is_black"]) else 1


def check_mix(noisy, clean, eps, alpha, what):
    """both arenas stand right after begin_move.  Returns the (game, agent, key) of every draw and the agents that searched."""
    draws = []
    for g in range(G):
        agent = searching_agent(noisy, g)
        if agent is None:
            continue
        key, nmv, eta, n = noisy.root_noise(g, agent)
        mv, _, _, pr = noisy.root_children(g, agent)
        cmv, _, _, cpr = clean.root_children(g, agent)
        assert n == mv.size == cmv.size, (what, g, n, mv.size, cmv.size)
        if n == 0:
            continue
        np.testing.assert_array_equal(nmv, mv, err_msg="%s: game %d: the recorded moves are the block order of the draw" % (what, g))
        np.testing.assert_array_equal(bits(eta), bits(capi.root_noise_of(key, n, alpha)), err_msg="%s: game %d eta" % (what, g))
        by_move = {int(m): p for m, p in zip(cmv, cpr)}
        assert sorted(by_move) == sorted(int(m) for m in mv), (what, g)
        want = mix(eps, np.array([by_move[int(m)] for m in mv], np.float32), eta)
        np.testing.assert_array_equal(bits(pr), bits(want), err_msg="%s: game %d priors" % (what, g))
        other = noisy.root_noise(g, 1 - agent)
        assert other[3] == 0 or other[0] != key                         # the tree that does not search draws nothing now
        draws.append((g, agent, key))
    return draws


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["komi5", "c4"])
def test_off_is_untouched(ctx, game):
    """never configured, on = 0, and on = 1 with eps = 0 (RandomCount = 0: the key drawn from the tree's stream is the only trace)"""
    kinds = (capi.INF_DUMMY, capi.INF_DUMMY) if game == "c4" else (capi.INF_HASH, capi.INF_HASH)
    arenas = [make(ctx, game, kinds=kinds, noise=n, RandomCount=0) for n in (None, dict(eps=0.25, alpha=0.3, on=False), dict(eps=0.0, alpha=0.3, on=True))]
    for ply in range(4):
        for a in arenas:
            move(a)
        assert_same(arenas[1], arenas[0], "on = 0, ply %d" % ply)
        assert_same(arenas[2], arenas[0], "eps = 0, ply %d" % ply)
    assert arenas[0].root_noise(0, 0)[3] == 0 and arenas[1].root_noise(0, 0)[3] == 0
    assert any(arenas[2].root_noise(g, agent)[3] > 0 for g in range(G) for agent in (0, 1))      # the ON path really ran
    for a in arenas:
        a.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
FRESH = [
    ("komi5", 0.25, 0.3, 1, "hash"), ("komi5", 0.25, 0.03, 1, "hash"), ("komi5", 0.5, 1.0, 1, "hash"), ("komi5", 1.0, 0.3, 1, "hash"),
    ("mnk6", 0.25, 0.3, 4, "hash"), ("mnk6", 0.25, 0.3, 1, "two"), ("go9", 0.25, 0.03, 1, "net"), ("c4", 0.25, 0.3, 1, "dummy"),
]


@pytest.mark.parametrize("game,eps,alpha,lanes,inf", FRESH, ids=["%s-%g-%g-l%d-%s" % c for c in FRESH])
def test_fresh_roots_the_mix_bit_for_bit(ctx, game, eps, alpha, lanes, inf):
    net = make_net(ctx) if inf == "net" else None
    kinds = {"hash": (capi.INF_HASH, capi.INF_HASH), "two": (capi.INF_HASH, capi.INF_DUMMY), "net": (capi.INF_NET, capi.INF_NET),
             "dummy": (capi.INF_DUMMY, capi.INF_DUMMY)}[inf]
    noisy = make(ctx, game, kinds=kinds, net=net, lanes=lanes, noise=dict(eps=eps, alpha=alpha))
    clean = make(ctx, game, kinds=kinds, net=net, lanes=lanes)
    assert noisy.get_root_noise() == {"eps": float(np.float32(eps)), "alpha": float(np.float32(alpha)), "on": True}
    for a in (noisy, clean):
        a.begin_move()
    draws = check_mix(noisy, clean, eps, alpha, "%s eps %g alpha %g" % (game, eps, alpha))
    assert len(draws) == G                                              # every fresh root was expanded by prepareRoot and got its draw
    assert len({k for _, _, k in draws}) == G, "keys repeat across trees"
    assert {agent for _, agent, _ in draws} == {0, 1}
    if eps == 1.0:                                                      # the priors ARE eta
        for g, agent, _ in draws:
            np.testing.assert_array_equal(bits(noisy.root_children(g, agent)[3]), bits(noisy.root_noise(g, agent)[2]))
    for a in (noisy, clean):
        a.simulate(a.mconf.Budget)
        a.end_move(True)
        a.close()
    if net is not None:
        net.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_reused_roots_and_checkpoints(ctx, tmp_path):
    """RandomCount = 4: randomizeChildren draws from the same per-tree stream as the noise key, and the stream is in the file"""
    eps, alpha = 0.25, 0.3
    conf = dict(RandomCount=4, RandomTemperature=1.0, Budget=32)
    path = str(tmp_path / "noise.ckpt")
    a = make(ctx, "komi5", noise=dict(eps=eps, alpha=alpha), **conf)
    for _ in range(3):
        move(a)
    a.save(path)
    b = make(ctx, "komi5", seed=977, opening=False, **conf)
    c = make(ctx, "komi5", seed=977, opening=False, **conf)
    b.load(path)
    c.load(path)
    c.set_root_noise(eps, alpha)
    assert c.root_noise(0, 0)[3] == 0 and c.root_noise(0, 1)[3] == 0    # the records are not in the file
    for x in (b, c):
        x.begin_move()
    draws = check_mix(c, b, eps, alpha, "after the load")
    assert draws
    boards, roots = c.last_prep_batch()
    assert roots < G, "no searched root kept its children: tree reuse was not exercised (%d roots evaluated)" % roots
    b.simulate(b.mconf.Budget)
    b.end_move(True)
    c.simulate(c.mconf.Budget)
    c.end_move(True)
    move(c)
    for _ in range(2):
        move(a)
    assert_same(c, a, "2 plies after the load")
    for x in (a, b, c):
        x.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_play_equals_the_three_call_rounds(ctx):
    noise = dict(eps=0.25, alpha=0.3)
    p = make(ctx, "mnk6", noise=noise, RandomCount=2, RandomTemperature=1.0)
    q = make(ctx, "mnk6", noise=noise, RandomCount=2, RandomTemperature=1.0)
    r = make(ctx, "mnk6", RandomCount=2, RandomTemperature=1.0)
    p.play(3)
    for _ in range(3):
        move(q)
        move(r)
    assert_same(p, q, "play(3) vs rounds")
    for g in range(G):
        for agent in (0, 1):
            assert p.root_noise(g, agent)[0] == q.root_noise(g, agent)[0]
    differs = any(not np.array_equal(bits(x), bits(y)) for g in range(G) for agent in (0, 1)
                  for x, y in zip(q.root_children(g, agent), r.root_children(g, agent)) if x.shape == y.shape)
    assert differs or any(not np.array_equal(q.history(g), r.history(g)) for g in range(G)), "the noise changed nothing"
    for x in (p, q, r):
        x.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
class Host:
    """the caller's game of a single tree (as tests/test_leaf_symmetry_gpu.py)"""

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


def by_move(children):
    mv, _, _, pr = children
    return {int(m): int(p) for m, p in zip(mv, bits(pr))}


def test_a_single_tree(ctx):
    S, budget, eps, alpha = 6, 24, 0.25, 0.3
    dev = A.Mcts(ctx, capi.GAME_MNK, S, S, 4, Budget=budget)
    dev.set_inferencer(capi.INF_HASH)
    dev.set_root_noise(eps, alpha)
    twin = A.Mcts(ctx, capi.GAME_MNK, S, S, 4, Budget=budget)
    twin.set_inferencer(capi.INF_HASH)
    assert dev.root_noise()[3] == 0
    host = Host(O.MNK, S, S, 4, 0.0)
    host.apply(O.BLACK, 14)
    for t in (dev, twin):
        t.set_game(**host.state_kw())
        t.search(O.WHITE)
    key, nmv, eta, n = dev.root_noise()
    assert n == S * S - 1 == dev.root_children()[0].size
    np.testing.assert_array_equal(bits(eta), bits(capi.root_noise_of(key, n, alpha)))
    clean = by_move(twin.root_children())
    pri = by_move(dev.root_children())
    want = mix(eps, np.array([clean[int(m)] for m in nmv], np.uint32).view(np.float32), eta)
    assert pri == {int(m): int(p) for m, p in zip(nmv, bits(want))}
    # the same position again, no move between: no new key, the priors stay
    best = dev.search(O.WHITE)
    assert dev.root_noise()[0] == key
    np.testing.assert_array_equal(bits(dev.root_noise()[2]), bits(eta))
    assert by_move(dev.root_children()) == pri
    # one more move: another root, another key
    host.apply(O.WHITE, best)
    dev.set_game(**host.state_kw())
    dev.search(O.BLACK)
    key2, _, eta2, n2 = dev.root_noise()
    assert key2 != key and n2 == S * S - 2
    np.testing.assert_array_equal(bits(eta2), bits(capi.root_noise_of(key2, n2, alpha)))
    dev.close()
    twin.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_the_arena_seed(ctx):
    """(the trees of game g of an arena seeded s share their streams with game g - 1 of an arena seeded s + 1 — the seeding the oracle
    parity of randomizeChildren fixed long ago — so the other seed here is further away than the arena is wide)"""
    noise = dict(eps=0.25, alpha=0.3)
    a, b, c = make(ctx, "komi5", noise=noise), make(ctx, "komi5", noise=noise), make(ctx, "komi5", seed=1005, noise=noise)
    for _ in range(3):
        for x in (a, b, c):
            move(x)
    assert_same(a, b, "same seed")
    ka = [a.root_noise(g, agent)[0] for g in range(G) for agent in (0, 1)]
    kb = [b.root_noise(g, agent)[0] for g in range(G) for agent in (0, 1)]
    kc = [c.root_noise(g, agent)[0] for g in range(G) for agent in (0, 1)]
    assert ka == kb and any(ka)
    assert not set(k for k in ka if k) & set(k for k in kc if k), "another arena seed drew the same keys"
    for x in (a, b, c):
        x.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_validation(ctx):
    L = capi.lib()
    a = make(ctx, "komi5")
    assert a.get_root_noise() == {"eps": 0.25, "alpha": float(np.float32(0.3)), "on": False}         # the defaults
    assert a.root_noise(0, 0)[3] == 0                                   # the observer before any draw, never configured
    a.set_root_noise(0.5, 0.75, True)
    have = a.get_root_noise()
    assert have == {"eps": 0.5, "alpha": 0.75, "on": True}
    assert a.root_noise(0, 0) [3] == 0 and a.root_noise(3, 1)[0] == 0   # configured, not yet searched
    nan, inf = float("nan"), float("inf")
    bad = [(0.25, 0.3, 2, 0), (0.25, 0.3, -1, 0), (-0.1, 0.3, 1, 0), (1.5, 0.3, 1, 0), (nan, 0.3, 1, 0), (inf, 0.3, 1, 0), (0.25, 0.0, 1, 0),
           (0.25, -1.0, 1, 0), (0.25, 1.5, 1, 0), (0.25, nan, 1, 0), (0.25, inf, 1, 0), (0.25, 0.3, 1, 1), (0.25, 0.3, 0, 7)]
    for eps, alpha, on, reserved in bad:
        conf = capi.NoiseConf(eps, alpha, on, reserved)
        assert L.agz_arena_set_root_noise(a.h, C.byref(conf)) == E_INVALID, (eps, alpha, on, reserved)
        assert b"agz_arena_set_root_noise" in L.agz_last_error()
        assert a.get_root_noise() == have
    assert L.agz_arena_set_root_noise(a.h, None) == E_INVALID and a.get_root_noise() == have
    ok = capi.NoiseConf(0.25, 0.3, 1, 0)
    assert L.agz_arena_set_root_noise(None, C.byref(ok)) == E_INVALID
    assert L.agz_arena_get_root_noise(a.h, None) == E_INVALID and L.agz_mcts_set_root_noise(None, C.byref(ok)) == E_INVALID
    a.begin_move()
    assert L.agz_arena_set_root_noise(a.h, C.byref(ok)) == E_STATE      # inside a move
    assert a.get_root_noise() == have
    # the observer: cap < n copies cap entries and reports n
    agent = searching_agent(a, 2)
    key, mv, eta, n = a.root_noise(2, agent)
    assert n > 3 and mv.size == n
    k3, mv3, eta3, n3 = a.root_noise(2, agent, cap=3)
    assert (k3, n3) == (key, n) and mv3.size == 3
    np.testing.assert_array_equal(mv3, mv[:3])
    np.testing.assert_array_equal(bits(eta3), bits(eta[:3]))
    k0, mv0, _, n0 = a.root_noise(2, agent, cap=0)
    assert (k0, n0, mv0.size) == (key, n, 0)
    cnt = C.c_int(0)
    for g, ag, cap in ((-1, 0, 4), (G, 0, 4), (0, 2, 4), (0, 0, -1)):
        assert L.agz_arena_root_noise(a.h, g, ag, None, None, None, cap, C.byref(cnt)) == E_INVALID, (g, ag, cap)
    assert L.agz_arena_root_noise(a.h, 0, 0, None, None, None, 0, None) == E_INVALID
    assert L.agz_arena_root_noise(a.h, 2, agent, None, None, None, 0, C.byref(cnt)) == 0 and cnt.value == n
    a.simulate(a.mconf.Budget)
    a.end_move(True)
    a.set_root_noise(on=False)                                          # off after on: allowed between moves
    assert a.get_root_noise()["on"] is False
    a.close()
