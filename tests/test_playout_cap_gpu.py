"""GPU: playout cap randomization (agz_arena_set_playout_cap, DESIGN.md §2 playout-cap).

The reference has no such rule, so the references here are (a) the host function agz_playout_cap_of — tests/test_playout_cap_cpu.py ties
it bit for bit to a pure-Python restatement of the declared definition — for every decision the arena reports, and (b) twin arenas from
the same seed for the searches: games never interact inside a search, so game g of a capped arena must equal game g of a replica that is
driven ply by ply with g's own decision (root noise on / off, the budget, record / no record) through the calls that exist without the
setting.  Everything is compared bit for bit with test_policy_target_gpu.assert_same (histories, boards, both roots' moves, visits,
blackScores bits and prior bits, counters, example rows per game).  AGZ_INF_HASH agents unless a test says otherwise.  Nothing here
depends on timing."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_policy_target_gpu import GAMES, assert_same, bits, make_net, rows_by_game, searching_agent

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE = -1, -6, -4
FULL, FAST = capi.CAP_FULL, capi.CAP_FAST
VISITS = capi.TARGET_VISITS
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
FAST_BUDGET = {"mnk3": 8, "c4": 8, "wq5": 16, "wq9": 24}          # against Budget 32, 32, 64, 100 (GAMES)
NOISE = (0.25, 0.3)


def make(ctx, game, seed=5, cap=None, noise=False, target=None, lanes=1, **over):
    """cap: None (never configured) or the keyword arguments of Arena.set_playout_cap"""
    c = dict(GAMES[game], **over)
    a = A.Arena(ctx, c.pop("kind"), c.pop("m"), c.pop("n"), seed=seed, **c)
    for agent in (0, 1):
        a.set_inferencer(agent, capi.INF_HASH)
    if lanes > 1:
        a.set_parallel(lanes)
    if target is not None:
        a.set_policy_target(*target)
    if noise:
        a.set_root_noise(*NOISE)
    if cap is not None:
        a.set_playout_cap(**cap)
    a.reset(np.array([g % 2 for g in range(a.n_games)], np.uint8))       # both agents get to search first somewhere
    return a


def move(a, k=None, record=True):
    a.begin_move()
    a.simulate(a.mconf.Budget if k is None else k)
    a.end_move(record)


def slot_keys(ctx, game, seed=5, **over):
    """the keys of the game slots of make(ctx, game, seed): read through the observer of a throw-away arena"""
    p = make(ctx, game, seed=seed, cap=dict(p_full=1.0, fast_budget=1), **over)
    p.begin_move()
    keys = [p.playout_cap(g)[0] for g in range(p.n_games)]
    p.simulate(1)
    p.end_move(False)
    p.close()
    assert len(set(keys)) == len(keys)
    return keys


def balanced_seed(keys, plies, p):
    """the first cap seed under which, over the (game, ply) pairs, at least two fifths are FULL and at least two fifths FAST (the tests
    ask for a third of the plies actually searched: a game may end before the last ply)"""
    n = len(keys) * plies
    for seed in range(1, 200):
        full = sum(capi.playout_cap_of(seed, key, ply, p) == FULL for key in keys for ply in range(plies))
        if 5 * full >= 2 * n and 5 * (n - full) >= 2 * n:
            return seed
    raise AssertionError("no balanced cap seed below 200")


def assert_game_same(a, b, g, what):
    """game g of two arenas: history, board, state, both roots, rows"""
    np.testing.assert_array_equal(a.history(g), b.history(g), err_msg="%s: history of game %d" % (what, g))
    (ba, sa), (bb, sb) = a.game(g), b.game(g)
    np.testing.assert_array_equal(ba, bb, err_msg="%s: board of game %d" % (what, g))
    assert sa == sb, (what, g, sa, sb)
    for agent in (0, 1):
        for x, y, name in zip(a.root_children(g, agent), b.root_children(g, agent), ("moves", "visits", "blackScores", "priors")):
            np.testing.assert_array_equal(bits(x), bits(y), err_msg="%s: game %d agent %d %s" % (what, g, agent, name))
    ra, rb = rows_by_game(a)[g], rows_by_game(b)[g]
    np.testing.assert_array_equal(bits(ra[0]), bits(rb[0]), err_msg="%s: policy rows of game %d" % (what, g))
    np.testing.assert_array_equal(bits(ra[1]), bits(rb[1]), err_msg="%s: values of game %d" % (what, g))


# ---- 1. off is untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", list(FAST_BUDGET))
def test_off_and_certainly_full_are_the_arena_without_the_setting(ctx, game):
    budget = GAMES[game]["Budget"]
    never = make(ctx, game)
    arenas = [make(ctx, game, cap=dict(p_full=0.25, fast_budget=FAST_BUDGET[game], on=False)),
              make(ctx, game, cap=dict(p_full=1.0, fast_budget=FAST_BUDGET[game], seed=3)),
              make(ctx, game, cap=dict(p_full=1.0, fast_budget=1, seed=3))]
    assert never.get_playout_cap() == {"p_full": 0.25, "fast_budget": 0, "on": False, "seed": 0}      # the defaults
    assert never.playout_cap(0) == (0, 0, -1, 0) and never.playout_cap_counts() == (0, 0)
    for x in [never] + arenas:
        x.play(4, True)
    for i, x in enumerate(arenas):
        assert_same(x, never, "%s arena %d" % (game, i))
    assert never.stats()["examples"] > 0 and never.stats()["sims_total"] == never.stats()["moves_played"] * budget
    assert arenas[0].playout_cap(0)[2] == -1 and arenas[0].playout_cap_counts() == (0, 0)
    assert arenas[2].playout_cap_counts() == (never.stats()["moves_played"], 0)
    for x in [never] + arenas:
        x.close()


# ---- 2. all fast -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", list(FAST_BUDGET))
def test_all_fast_is_the_short_search_without_noise_and_without_rows(ctx, game):
    fast = FAST_BUDGET[game]
    a = make(ctx, game, cap=dict(p_full=0.0, fast_budget=fast, seed=9), noise=True, target=(VISITS, 1.0))
    twin = make(ctx, game)
    a.play(4, True)
    for ply in range(4):
        move(twin, fast, record=False)
    assert_same(a, twin, "%s all fast" % game)
    st = a.stats()
    assert st["examples"] == 0 and st["sims_total"] == st["moves_played"] * fast
    assert a.playout_cap_counts() == (0, st["moves_played"])
    for g in range(a.n_games):
        for agent in (0, 1):
            assert a.root_noise(g, agent)[3] == 0, "a fast search drew root noise"
    a.close()
    twin.close()


# ---- 3. the decision -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,p", [("mnk3", 0.5), ("c4", 0.25), ("wq5", 0.75)])
def test_every_decision_is_the_host_function(ctx, game, p):
    fast, budget, seed = FAST_BUDGET[game], GAMES[game]["Budget"], 0xFEEDC0DE12345
    a = make(ctx, game, cap=dict(p_full=p, fast_budget=fast, seed=seed))
    assert a.get_playout_cap() == {"p_full": p, "fast_budget": fast, "on": True, "seed": seed}
    keys = {}
    tally = [0, 0]
    for ply in range(6):
        a.begin_move()
        for g in range(a.n_games):
            if searching_agent(a, g) is None:
                continue
            key, cply, kind, b = a.playout_cap(g)
            assert keys.setdefault(g, key) == key                       # a slot keeps its key until it restarts
            assert cply == len(a.history(g)) == ply
            assert kind == capi.playout_cap_of(seed, key, cply, p), (g, ply)
            assert b == (budget if kind == FULL else fast)
            tally[kind] += 1
        a.simulate(budget)
        a.end_move(True)
        assert a.playout_cap_counts() == tuple(tally)
    assert len(set(keys.values())) == a.n_games
    assert a.stats()["sims_total"] == tally[FULL] * budget + tally[FAST] * fast
    a.close()


# ---- 4. / 5. mixed plies ---------------------------------------------------------------------------------------------------------
def mixed(ctx, game, plies, lanes=1, **over):
    """the capped arena against one replica per game, driven with that game's decisions"""
    p = 0.5
    fast = over.pop("fast", FAST_BUDGET[game])
    keys = slot_keys(ctx, game, **over)
    seed = balanced_seed(keys, plies, p)
    a = make(ctx, game, cap=dict(p_full=p, fast_budget=fast, seed=seed), noise=True, target=(VISITS, 1.0), lanes=lanes, **over)
    budget = a.mconf.Budget
    decisions = []                                                      # [ply][g] = (kind, budget) or None for a finished game
    for ply in range(plies):
        a.begin_move()
        row = []
        for g in range(a.n_games):
            if searching_agent(a, g) is None:
                row.append(None)
                continue
            key, cply, kind, b = a.playout_cap(g)
            assert key == keys[g] and kind == capi.playout_cap_of(seed, key, cply, p) and b == (budget if kind == FULL else fast)
            row.append((kind, b))
        decisions.append(row)
        a.simulate(budget)
        a.end_move(True)
    made = [d for row in decisions for d in row if d is not None]
    n_full = sum(d[0] == FULL for d in made)
    assert len(made) >= a.n_games * plies * 2 // 3, "most games ended early: the plies were not exercised"
    assert 3 * n_full >= len(made) and 3 * (len(made) - n_full) >= len(made), (n_full, len(made))
    assert a.stats()["sims_total"] == sum(d[1] for d in made)
    for g in range(a.n_games):
        r = make(ctx, game, target=(VISITS, 1.0), lanes=lanes, **over)
        for ply in range(plies):
            d = decisions[ply][g]
            kind, b = d if d is not None else (FAST, fast)              # (game g is over: whatever the other games of the replica do)
            r.set_root_noise(NOISE[0], NOISE[1], on=(kind == FULL))
            move(r, b, record=(kind == FULL))
        assert_game_same(a, r, g, "%s lanes %d game %d" % (game, lanes, g))
        for agent in (0, 1):                                            # the noise record of either tree: the same draws, nothing drawn on fast plies
            na, nr = a.root_noise(g, agent), r.root_noise(g, agent)
            assert na[0] == nr[0] and na[3] == nr[3]
            np.testing.assert_array_equal(bits(na[2]), bits(nr[2]))
        r.close()
    if game == "wq9":
        assert max(a.root_children(g, ag)[0].size for g in range(a.n_games) for ag in (0, 1)) > 64
    a.close()


@pytest.mark.parametrize("game", list(FAST_BUDGET))
def test_a_game_of_a_mixed_arena_is_the_game_driven_with_its_own_decisions(ctx, game):
    mixed(ctx, game, 6)


@pytest.mark.parametrize("game", ["mnk3", "wq5"])
def test_mixed_plies_in_lane_rounds_with_a_partial_boundary_round(ctx, game):
    """4 lanes, budgets 30 / 10: a fast game's rounds are 4, 4, 2 — the round that crosses fast_budget runs two of its four lanes"""
    mixed(ctx, game, 6, lanes=4, Budget=30, fast=10)


@pytest.mark.parametrize("game", ["mnk3", "wq5"])
def test_all_fast_in_lane_rounds_still_runs_the_round_that_crosses_fast_budget(ctx, game):
    """4 lanes, budgets 30 / 10, p_full = 0: no game is FULL, and the round that starts at simulation 8 still owes every game two lanes.
    A twin driven simulate(10) plays the same games; simulate in chunks of 3 (rounds 3, 3, 3, then 1 of 3) must give them as well"""
    fast = 10
    cap = dict(p_full=0.0, fast_budget=fast, seed=9)
    a = make(ctx, game, cap=cap, noise=True, target=(VISITS, 1.0), lanes=4, Budget=30)
    c = make(ctx, game, cap=cap, lanes=4, Budget=30)
    twin, twin3 = make(ctx, game, lanes=4, Budget=30), make(ctx, game, lanes=4, Budget=30)
    a.play(4, True)
    for ply in range(4):
        move(twin, fast, record=False)
        for x, k in ((c, 30), (twin3, fast)):                           # the same chunks: a lane round never spans two simulate calls
            x.begin_move()
            for done in range(0, k, 3):
                x.simulate(min(3, k - done))
            x.end_move(False)
    assert_same(a, twin, "%s all fast, 4 lanes" % game)
    assert_same(c, twin3, "%s all fast, 4 lanes, chunks of 3" % game)
    for x in (a, c):
        st = x.stats()
        assert st["examples"] == 0 and st["sims_total"] == st["moves_played"] * fast
        assert x.playout_cap_counts() == (0, st["moves_played"])
    for x in (a, c, twin, twin3):
        x.close()


# ---- 6. a real network: the compacted tail ---------------------------------------------------------------------------------------
def net_arena(ctx, net, S, G, budget, seed, cap):
    a = A.Arena(ctx, capi.GAME_WQ, S, S, 0, 7.5, encoder=capi.ENC_WQ, n_games=G, seed=seed, Budget=budget)
    for agent in (0, 1):
        a.set_inferencer(agent, capi.INF_NET, net)
    a.set_policy_target(VISITS, 1.0)
    a.set_playout_cap(**cap)
    a.reset(np.array([(i % 2) == 1 for i in range(G)], dtype=np.uint8))
    a.random_moves(np.random.default_rng(seed).integers(0, 12, size=G).astype(np.int32), seed)
    return a


def test_the_tail_runs_on_the_packed_batch_of_the_full_games(ctx):
    S, G, budget, fast, p = 19, 64, 16, 4, 0.25
    net = A.Net(ctx, 64, 2, 64, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(1337)
    net.commit()
    cap = dict(p_full=p, fast_budget=fast, seed=11)
    packed, whole = net_arena(ctx, net, S, G, budget, 31, cap), net_arena(ctx, net, S, G, budget, 31, cap)
    whole.set_cap_compact(False)
    smaller = 0
    for ply in range(3):
        n_full = None
        for a in (packed, whole):
            a.begin_move()
            kinds = [a.playout_cap(g)[2] for g in range(G)]
            assert n_full in (None, kinds.count(FULL))
            n_full = kinds.count(FULL)
            a.simulate(fast)
            assert a.last_cap_batch() == (0, 0)                          # a step within fast_budget is no tail step
            a.simulate(budget - fast)
        assert 0 < n_full < G
        want = net.min_same_batch(n_full, G)
        print("ply %d: %d full games of %d, tail batch %d" % (ply, n_full, G, want))
        assert packed.last_cap_batch() == (want, n_full)
        assert whole.last_cap_batch() == (G, n_full)
        smaller += want < G
        for a in (packed, whole):
            a.end_move(True)
        assert_same(packed, whole, "ply %d" % ply)
    assert smaller > 0, "no tail step ran on a batch below G: the compaction was not exercised"
    assert packed.stats()["examples"] == packed.playout_cap_counts()[0] > 0
    # a move without a FULL game enqueues no tail step
    packed.set_playout_cap(p_full=0.0, fast_budget=fast, seed=11)
    s0, j0, _ = packed.split_steps()
    sims0 = packed.stats()["sims_total"]
    move(packed, budget)
    s1, j1, _ = packed.split_steps()
    assert (s1 + j1) - (s0 + j0) == fast
    assert packed.last_cap_batch() == (0, 0)
    assert packed.stats()["sims_total"] - sims0 == G * fast
    for a in (packed, whole):
        a.close()
    net.close()


# ---- 7. split step ---------------------------------------------------------------------------------------------------------------
def test_split_head_steps_and_joined_tail_steps(ctx):
    """tests/test_split_step_gpu.py's small shape (416 games of 9x9 Go, K = 256, four blocks, two tower queues): within fast_budget the
    capped arena takes the split step, past it the joined tail step; against set_split(0) everything is bit-identical"""
    S, G, budget, fast, plies = 9, 416, 8, 4, 3
    net = make_net(ctx, S, 256, 4)
    cap = dict(p_full=0.5, fast_budget=fast, seed=5)
    arenas = []
    for m in (0, 1):
        a = net_arena(ctx, net, S, G, budget, 31, cap)
        a.set_split(m)
        arenas.append(a)
    joined, split = arenas
    for ply in range(plies):
        for a in arenas:
            move(a, budget)
    assert_same(split, joined, "%d plies" % plies)
    js, ss = joined.split_steps(), split.split_steps()
    assert js[0] == 0 and js[1] == plies * budget, js
    assert ss[0] == plies * fast and ss[1] == plies * (budget - fast), ss
    full, fastn = split.playout_cap_counts()
    assert full > 0 and fastn > 0 and split.stats()["examples"] == full
    for a in arenas:
        a.close()
    net.close()


# ---- 8. checkpoint ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_continuation(ctx, tmp_path):
    game, p = "wq5", 0.5
    fast, budget = FAST_BUDGET[game], GAMES[game]["Budget"]
    conf = dict(RandomCount=6, RandomTemperature=1.0)
    cap = dict(p_full=p, fast_budget=fast, seed=balanced_seed(slot_keys(ctx, game, **conf), 5, p))
    path = str(tmp_path / "cap.ckpt")
    a = make(ctx, game, cap=cap, noise=True, target=(VISITS, 0.5), **conf)
    for ply in range(2):
        move(a)
    a.save(path)
    b, c = make(ctx, game, seed=977, **conf), make(ctx, game, seed=977, **conf)
    for x in (b, c):
        x.load(path)
        assert x.get_playout_cap()["on"] is False                       # the setting is not in the file
        assert x.playout_cap(0)[2] == -1 and x.playout_cap_counts() == (0, 0)
    b.set_playout_cap(**cap)
    b.set_root_noise(*NOISE)
    b.set_policy_target(VISITS, 0.5)
    before = a.playout_cap_counts()
    for ply in range(3):
        move(a)
        move(b)
    assert_same(b, a, "3 plies after the load")
    after = a.playout_cap_counts()
    assert b.playout_cap_counts() == (after[0] - before[0], after[1] - before[1])
    for g in range(a.n_games):
        assert b.playout_cap(g) == a.playout_cap(g)
    sims = c.stats()["sims_total"]
    live = sum(searching_agent(c, g) is not None for g in range(c.n_games))
    move(c)                                                             # without the setting a loaded arena searches every game in full
    assert c.stats()["sims_total"] - sims == live * budget and c.playout_cap_counts() == (0, 0)
    for x in (a, b, c):
        x.close()


# ---- 9. continuous self-play -----------------------------------------------------------------------------------------------------
def test_selfplay_with_restarts(ctx):
    game, p, tau = "mnk3", 0.5, 1.0
    fast, budget, seed = FAST_BUDGET[game], GAMES[game]["Budget"], 77
    keys0 = slot_keys(ctx, game)
    cap = dict(p_full=p, fast_budget=fast, seed=seed)
    s = make(ctx, game, cap=cap, target=(VISITS, tau))
    s.selfplay(24)
    st = s.stats()
    full, fastn = s.playout_cap_counts()
    assert st["games_finished"] >= 24 and full > 0 and fastn > 0
    assert full + fastn == st["moves_played"]
    assert st["examples"] == full and st.get("examples_dropped", 0) == 0   # mnk: every searched root has a visited child
    assert st["sims_total"] == full * budget + fastn * fast
    restarted = 0
    for g in range(s.n_games):
        key, ply, kind, b = s.playout_cap(g)
        steps = [k for k in range(12) if (keys0[g] + k * GOLD) & M64 == key]
        assert len(steps) == 1, "slot %d: the key is not the slot's key advanced once per restart" % g
        restarted += steps[0] > 0
        assert kind == capi.playout_cap_of(seed, key, ply, p) and b == (budget if kind == FULL else fast)
    assert restarted > 0
    # the first game of every slot, driven by rounds: its FULL plies are the slot's first rows, bit for bit
    q = make(ctx, game, cap=cap, target=(VISITS, tau))
    n_full = [0] * q.n_games
    plies = 0
    while any(searching_agent(q, g) is not None for g in range(q.n_games)):
        q.begin_move()
        for g in range(q.n_games):
            if searching_agent(q, g) is not None:
                n_full[g] += q.playout_cap(g)[2] == FULL
        q.simulate(budget)
        q.end_move(True)
        plies += 1
        assert plies <= 9
    rows_s, rows_q = rows_by_game(s), rows_by_game(q)
    assert sum(r[0].shape[0] for r in rows_s.values()) == full
    for g in range(q.n_games):
        k = rows_q[g][0].shape[0]
        assert k == n_full[g] and rows_s[g][0].shape[0] >= k
        np.testing.assert_array_equal(bits(rows_s[g][0][:k]), bits(rows_q[g][0]), err_msg="first game of slot %d" % g)
        np.testing.assert_array_equal(bits(rows_s[g][1][:k]), bits(rows_q[g][1]), err_msg="labels of the first game of slot %d" % g)
    # every slot across its restarts: the j-th game of slot g has the key keys0[g] + j GOLD, and the plies of a recorded row can be read off
    # its planes (the stones on the board).  The slot's rows, in the order recorded, must be the FULL plies below the length of game 0,
    # then of game 1, ... for SOME game lengths (5 .. 9 moves; the last game may be unfinished): no row sits on a FAST ply
    planes, _, _, gidx = s.examples()
    stones = (np.abs(planes.reshape(-1, 2, 9)[:, 0]) == 1.0).sum(axis=1)
    for g in range(s.n_games):
        key, last_ply, _, _ = s.playout_cap(g)
        n_games = [k for k in range(12) if (keys0[g] + k * GOLD) & M64 == key][0] + 1
        plies = [int(x) for x in stones[gidx == g]]
        full_of = [[p_ for p_ in range(9) if capi.playout_cap_of(seed, (keys0[g] + j * GOLD) & M64, p_, p) == FULL] for j in range(n_games)]

        def parses(j, at):
            if j == n_games:
                return at == len(plies)
            lengths = range(5, 10) if j < n_games - 1 else [last_ply + 1]        # (the game of the slot's last search: plies 0 .. last_ply)
            for length in lengths:
                want = [p_ for p_ in full_of[j] if p_ < length]
                if plies[at:at + len(want)] == want and parses(j + 1, at + len(want)):
                    return True
            return False

        assert parses(0, 0), "slot %d: rows at plies %s are not the FULL plies %s of its %d games" % (g, plies, full_of, n_games)
    for x in (s, q):
        x.close()


# ---- 10. validation --------------------------------------------------------------------------------------------------------------
def test_validation(ctx):
    L = capi.lib()
    a = make(ctx, "mnk3")
    budget = a.mconf.Budget
    a.set_playout_cap(p_full=0.5, fast_budget=8, seed=123)
    have = a.get_playout_cap()
    assert have == {"p_full": 0.5, "fast_budget": 8, "on": True, "seed": 123}
    nan, inf = float("nan"), float("inf")
    bad = [(0.5, 8, 2, 0), (0.5, 8, -1, 0), (-0.25, 8, 1, 0), (1.5, 8, 1, 0), (nan, 8, 1, 0), (inf, 8, 1, 0), (-inf, 8, 0, 0), (nan, 8, 0, 0),
           (0.5, 8, 1, 1), (0.5, 8, 0, -1), (0.5, 0, 1, 0), (0.5, -3, 1, 0), (0.5, budget + 1, 1, 0)]
    for p, fast, on, reserved in bad:
        conf = capi.PlayoutCapConf(p, fast, on, reserved, 5)
        assert L.agz_arena_set_playout_cap(a.h, C.byref(conf)) == E_INVALID, (p, fast, on, reserved)
        assert b"agz_arena_set_playout_cap" in L.agz_last_error()
        assert a.get_playout_cap() == have
    ok = capi.PlayoutCapConf(0.5, budget, 1, 0, 5)
    assert L.agz_arena_set_playout_cap(a.h, None) == E_INVALID and a.get_playout_cap() == have
    assert L.agz_arena_set_playout_cap(None, C.byref(ok)) == E_INVALID
    assert L.agz_arena_get_playout_cap(a.h, None) == E_INVALID and L.agz_arena_get_playout_cap(None, C.byref(ok)) == E_INVALID
    assert L.agz_arena_playout_cap(a.h, a.n_games, None, None, None, None) == E_INVALID
    assert L.agz_arena_playout_cap(a.h, -1, None, None, None, None) == E_INVALID
    assert L.agz_arena_playout_cap(a.h, 0, None, None, None, None) == 0 and L.agz_arena_playout_cap_counts(a.h, None, None) == 0
    a.begin_move()
    assert L.agz_arena_set_playout_cap(a.h, C.byref(ok)) == E_STATE       # inside a move
    assert a.get_playout_cap() == have
    a.simulate(budget)
    a.end_move(True)
    a.set_playout_cap(p_full=1.0, fast_budget=budget)                      # fast_budget == Budget is allowed
    a.set_playout_cap(on=False)                                            # off: fast_budget is not looked at
    assert a.get_playout_cap() == {"p_full": 0.25, "fast_budget": 0, "on": False, "seed": 0}
    a.close()
    z = make(ctx, "mnk3", Budget=0)                                        # nothing to cap
    have = z.get_playout_cap()
    conf = capi.PlayoutCapConf(0.5, 1, 1, 0, 0)
    assert L.agz_arena_set_playout_cap(z.h, C.byref(conf)) == E_UNSUPPORTED and z.get_playout_cap() == have
    z.set_playout_cap(on=False)
    z.close()
