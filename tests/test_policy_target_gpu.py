"""GPU: root visit counts as policy targets (agz_arena_set_policy_target, DESIGN.md §2 visit-target).

The reference has no such target, so the references here are (a) the host function agz_visit_target_of — tests/test_policy_target_cpu.py
ties it bit for bit to a pure-Python restatement of the declared definition — applied to the root children read back right before
agz_arena_end_move, and (b) twin arenas from the same seed for everything that must stay bit-identical: the search under either kind, the
default, the checkpoint continuation, selfplay / the split step against the plain rounds.  Rows, roots (children, visits, blackScores
bits, prior bits), histories and counters are compared bit for bit.  AGZ_INF_HASH agents unless a test says otherwise.  Nothing here
depends on timing."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
REF, VISITS = capi.TARGET_REFERENCE, capi.TARGET_VISITS
STAT_KEYS = ("sims_total", "sims_nonnull", "nn_evals", "moves_played", "games_finished", "tree_full")

GAMES = {
    "mnk3": dict(kind=capi.GAME_MNK, m=3, n=3, k=3, komi=0.0, encoder=capi.ENC_TWOPLANE, n_games=8, Budget=32),
    "c4": dict(kind=capi.GAME_C4, m=6, n=7, k=4, komi=0.0, encoder=capi.ENC_TWOPLANE, n_games=4, Budget=32),
    "wq5": dict(kind=capi.GAME_WQ, m=5, n=5, k=0, komi=5.5, encoder=capi.ENC_WQ, n_games=4, Budget=64),
    "wq9": dict(kind=capi.GAME_WQ, m=9, n=9, k=0, komi=5.5, encoder=capi.ENC_WQ, n_games=2, Budget=100),
    "wq19": dict(kind=capi.GAME_WQ, m=19, n=19, k=0, komi=7.5, encoder=capi.ENC_WQ, n_games=1, Budget=64),
}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def make(ctx, game, seed=5, target=None, **over):
    """target: None (never configured) or (kind, temperature)"""
    c = dict(GAMES[game], **over)
    a = A.Arena(ctx, c.pop("kind"), c.pop("m"), c.pop("n"), seed=seed, **c)
    for agent in (0, 1):
        a.set_inferencer(agent, capi.INF_HASH)
    if target is not None:
        a.set_policy_target(*target)
    a.reset(np.array([g % 2 for g in range(a.n_games)], np.uint8))       # both agents get to search first somewhere
    return a


def searching_agent(a, g):
    _, st = a.game(g)
    if st["ended"]:
        return None
    return 0 if (st["to_move"] == capi.BLACK) == bool(st["a_is_black"]) else 1


def rows_by_game(a):
    """game -> (policy rows, values) in the order recorded (k_end_move hands rows out through an atomic counter: compare per game)"""
    _, policy, value, gidx = a.examples()
    return {g: (policy[gidx == g], value[gidx == g]) for g in range(a.n_games)}


def checked_move(a, tau, what, record=True):
    """one begin / simulate / end round of a TARGET_VISITS arena: the newest row of every game is agz_visit_target_of of the mover's root
    children as they stood before end_move; a game without a visited child gets no row.  Returns the number of rows checked."""
    a.begin_move()
    a.simulate(a.mconf.Budget)
    roots = {}
    for g in range(a.n_games):
        agent = searching_agent(a, g)
        if agent is not None:
            mv, vis, _, _ = a.root_children(g, agent)
            roots[g] = (mv, vis)
    before = {g: r[0].shape[0] for g, r in rows_by_game(a).items()}
    a.end_move(record)
    after = rows_by_game(a)
    checked = 0
    for g in range(a.n_games):
        grew = after[g][0].shape[0] - before[g]
        if not record or g not in roots or roots[g][1].size == 0 or int(roots[g][1].max()) == 0:
            assert grew == 0, (what, g, grew)
            continue
        assert grew == 1, "%s: game %d recorded %d rows on a searched ply" % (what, g, grew)
        mv, vis = roots[g]
        want = capi.visit_target_of(mv, vis, a.action_space, tau)
        np.testing.assert_array_equal(bits(after[g][0][-1]), bits(want), err_msg="%s: game %d, %d children" % (what, g, mv.size))
        checked += 1
    return checked


def assert_same(a, b, what, examples=True):
    for g in range(a.n_games):
        np.testing.assert_array_equal(a.history(g), b.history(g), err_msg="%s: history of game %d" % (what, g))
        (ba, sa), (bb, sb) = a.game(g), b.game(g)
        np.testing.assert_array_equal(ba, bb, err_msg="%s: board of game %d" % (what, g))
        assert sa == sb, (what, g, sa, sb)
        for agent in (0, 1):
            for x, y, name in zip(a.root_children(g, agent), b.root_children(g, agent), ("moves", "visits", "blackScores", "priors")):
                np.testing.assert_array_equal(bits(x), bits(y), err_msg="%s: game %d agent %d %s" % (what, g, agent, name))
    sa, sb = a.stats(), b.stats()
    for key in STAT_KEYS:
        assert sa[key] == sb[key], (what, key, sa[key], sb[key])
    if examples:
        assert sa["examples"] == sb["examples"], (what, sa["examples"], sb["examples"])
        ea, eb = a.examples(), b.examples()
        oa, ob = np.argsort(ea[3], kind="stable"), np.argsort(eb[3], kind="stable")
        for x, y, name in zip(ea, eb, ("planes", "policy", "value", "game")):
            np.testing.assert_array_equal(bits(x[oa]), bits(y[ob]), err_msg="%s: example %s" % (what, name))


# ---- 1. row parity ---------------------------------------------------------------------------------------------------------------
PARITY = [(game, tau, {}) for game in ("mnk3", "c4", "wq5", "wq9", "wq19") for tau in (1.0, 0.5, 2.0)]
PARITY.append(("wq5", 0.5, dict(RandomCount=10, RandomTemperature=1.0)))   # randomizeChildren reorders the block in the same kernel
PARITY.append(("mnk3", 0.25, dict(RandomCount=4, RandomTemperature=0.5)))


@pytest.mark.parametrize("game,tau,over", PARITY, ids=["%s-%g%s" % (g, t, "-random" if o else "") for g, t, o in PARITY])
def test_the_row_is_the_host_definition_of_the_read_back_root(ctx, game, tau, over):
    a = make(ctx, game, target=(VISITS, tau), **over)
    assert a.get_policy_target() == {"kind": VISITS, "temperature": tau}
    total = 0
    for ply in range(3):                                                # plies 1 and 2 search re-rooted trees with carried visits
        total += checked_move(a, tau, "%s tau %g ply %d" % (game, tau, ply))
    assert total == 3 * a.n_games, total                                # every game recorded on every ply
    planes, policy, value, gidx = a.examples()
    assert policy.shape == (total, a.action_space + 1)
    if game.startswith("wq"):                                           # the Pass child exists and lands in the last entry
        mv, vis, _, _ = a.root_children(0, 0)
        assert capi.PASS in mv
    if game == "wq9":
        assert a.root_children(0, 0)[0].size > 64                       # more than one pass of the wavefront over the children
    if game == "wq19":
        assert a.root_children(0, 0)[0].size > 320                      # six children per lane
    a.close()


def test_a_row_with_a_visited_pass_child_carries_it_in_the_last_entry(ctx):
    """wq 5x5, PREFER_PASS so that a searched Pass is not replaced: over a few plies some root has a Pass child with visits"""
    a = make(ctx, "wq5", target=(VISITS, 1.0), PassPreference=capi.PREFER_PASS)
    seen = 0
    for ply in range(4):
        a.begin_move()
        a.simulate(a.mconf.Budget)
        roots = {g: a.root_children(g, searching_agent(a, g))[:2] for g in range(a.n_games) if searching_agent(a, g) is not None}
        a.end_move(True)
        rows = rows_by_game(a)
        for g, (mv, vis) in roots.items():
            vp = int(vis[mv == capi.PASS][0]) if capi.PASS in mv else 0
            if vp > 0:
                seen += 1
                assert rows[g][0][-1][a.action_space] == np.float32(np.float64(vp) / np.float64(vis.astype(np.float64).sum()))
    assert seen > 0, "no root had a visited Pass child: the last entry was not exercised"
    a.close()


# ---- 2. the search is untouched --------------------------------------------------------------------------------------------------
def test_the_kind_changes_rows_and_their_number_and_nothing_else(ctx):
    """wq 5x5 to the end under PREFER_PASS (a searched Pass is played, games end by two passes or at max_moves).  REFERENCE and VISITS
    arenas of one seed: the same roots on every ply, the same games; VISITS has one row per searched ply, REFERENCE drops the Pass plies."""
    conf = dict(PassPreference=capi.PREFER_PASS, Budget=32)
    r, v = make(ctx, "wq5", target=(REF, 1.0), **conf), make(ctx, "wq5", target=(VISITS, 1.0), **conf)
    G = v.n_games
    movers = {g: [] for g in range(G)}                                  # the colour to move at every recorded row of the VISITS arena
    plies = 0
    while any(searching_agent(v, g) is not None for g in range(G)):
        assert plies < 2 * 25 + 2, "a game did not end at max_moves"
        for x in (r, v):
            x.begin_move()
            x.simulate(x.mconf.Budget)
        for g in range(G):
            agent = searching_agent(v, g)
            assert agent == searching_agent(r, g)
            if agent is None:
                continue
            cr, cv = r.root_children(g, agent), v.root_children(g, agent)
            for x, y, name in zip(cr, cv, ("moves", "visits", "blackScores", "priors")):
                np.testing.assert_array_equal(bits(x), bits(y), err_msg="ply %d game %d %s" % (plies, g, name))
            if cv[1].size and int(cv[1].max()) > 0:
                movers[g].append(v.game(g)[1]["to_move"])
        for x in (r, v):
            x.end_move(True)
        plies += 1
        assert_same(r, v, "ply %d" % plies, examples=False)
    rows_r, rows_v = rows_by_game(r), rows_by_game(v)
    passes = sum(int((v.history(g) == capi.PASS).sum()) for g in range(G))
    assert passes > 0, "no Pass was played: the difference in the example count was not exercised"
    n_r, n_v = sum(x[0].shape[0] for x in rows_r.values()), sum(x[0].shape[0] for x in rows_v.values())
    assert n_v == sum(len(m) for m in movers.values()) == v.stats()["examples"]
    assert n_v - passes <= n_r < n_v, (n_r, n_v, passes)                # (a Pass ply whose board hash met a board move earlier keeps its reference row)
    for g in range(G):
        _, st = v.game(g)
        assert st["ended"]
        policy, value = rows_v[g]
        assert policy.shape[0] == len(movers[g])
        want = [0.0 if st["winner"] == capi.NONE else (1.0 if m == st["winner"] else -1.0) for m in movers[g]]
        np.testing.assert_array_equal(value, np.array(want, np.float32), err_msg="labels of game %d" % g)
        assert set(np.unique(rows_r[g][1]).tolist()) <= {-1.0, 0.0, 1.0}
        assert (np.abs(policy.astype(np.float64).sum(axis=1) - 1.0) <= 26 * 2.0 ** -24).all()
    r.close()
    v.close()


# ---- 3. the default --------------------------------------------------------------------------------------------------------------
def test_default_kind_and_validation(ctx):
    L = capi.lib()
    never = make(ctx, "wq5", PassPreference=capi.PREFER_PASS)
    zero = make(ctx, "wq5", target=(REF, 2.0), PassPreference=capi.PREFER_PASS)      # kind 0: the temperature is stored and not used
    assert never.get_policy_target() == {"kind": REF, "temperature": 1.0}            # the defaults
    assert zero.get_policy_target() == {"kind": REF, "temperature": 2.0}
    for ply in range(4):
        for a in (never, zero):
            a.begin_move()
            a.simulate(a.mconf.Budget)
            a.end_move(True)
        assert_same(zero, never, "kind 0, ply %d" % ply)
    assert never.stats()["examples"] > 0
    zero.close()
    a = never
    a.set_policy_target(VISITS, 0.5)
    have = a.get_policy_target()
    assert have == {"kind": VISITS, "temperature": 0.5}
    nan, inf = float("nan"), float("inf")
    bad = [(2, 1.0, 0, 0), (-1, 1.0, 0, 0), (VISITS, 0.0, 0, 0), (VISITS, -0.0, 0, 0), (VISITS, -1.0, 0, 0), (VISITS, nan, 0, 0), (VISITS, inf, 0, 0),
           (VISITS, -inf, 0, 0), (REF, 0.0, 0, 0), (REF, nan, 0, 0), (VISITS, 1.0, 1, 0), (VISITS, 1.0, 0, 1), (REF, 1.0, 0, -1)]
    for kind, tau, r0, r1 in bad:
        conf = capi.TargetConf(kind, tau, (C.c_int32 * 2)(r0, r1))
        assert L.agz_arena_set_policy_target(a.h, C.byref(conf)) == E_INVALID, (kind, tau, r0, r1)
        assert b"agz_arena_set_policy_target" in L.agz_last_error()
        assert a.get_policy_target() == have
    assert L.agz_arena_set_policy_target(a.h, None) == E_INVALID and a.get_policy_target() == have
    ok = capi.TargetConf(REF, 1.0, (C.c_int32 * 2)(0, 0))
    assert L.agz_arena_set_policy_target(None, C.byref(ok)) == E_INVALID
    assert L.agz_arena_get_policy_target(a.h, None) == E_INVALID and L.agz_arena_get_policy_target(None, C.byref(ok)) == E_INVALID
    a.begin_move()
    assert L.agz_arena_set_policy_target(a.h, C.byref(ok)) == E_STATE      # inside a move
    assert a.get_policy_target() == have
    a.simulate(a.mconf.Budget)
    a.end_move(True)
    a.set_policy_target(REF)                                               # back to the reference kind between moves
    assert a.get_policy_target() == {"kind": REF, "temperature": 1.0}
    a.close()


# ---- 4. the other paths ----------------------------------------------------------------------------------------------------------
def test_play_equals_the_three_call_rounds(ctx):
    p, q = make(ctx, "wq5", target=(VISITS, 0.5)), make(ctx, "wq5", target=(VISITS, 0.5))
    p.play(3)
    for ply in range(3):
        checked_move(q, 0.5, "rounds, ply %d" % ply)
    assert_same(p, q, "play(3) vs rounds")
    p.close()
    q.close()


def test_selfplay_with_restarts(ctx):
    """agz_arena_selfplay: 8 slots of mnk 3x3 until 24 games are done.  Restarts put later games into the slots, which plain rounds cannot
    follow, so: (a) the first game of every slot is the game the checked rounds play from the same seed — its rows are theirs, bit for bit;
    (b) every row of every later game is a distribution over EMPTY cells of the position it was recorded with; (c) one row per move played,
    and a REFERENCE twin plays the same games."""
    tau = 2.0
    s = make(ctx, "mnk3", target=(VISITS, tau))
    s.selfplay(24)
    st = s.stats()
    assert st["games_finished"] >= 24
    assert st["examples"] == st["moves_played"] and st.get("examples_dropped", 0) == 0      # mnk: every searched root has visited children
    twin = make(ctx, "mnk3", target=(REF, 1.0))
    twin.selfplay(24)
    for key in STAT_KEYS:
        assert twin.stats()[key] == st[key], key
    q = make(ctx, "mnk3", target=(VISITS, tau))
    ply = 0
    while any(searching_agent(q, g) is not None for g in range(q.n_games)):
        checked_move(q, tau, "rounds, ply %d" % ply)
        ply += 1
        assert ply <= 9
    rows_s, rows_q = rows_by_game(s), rows_by_game(q)
    for g in range(q.n_games):
        k = rows_q[g][0].shape[0]
        assert 5 <= k <= 9 and rows_s[g][0].shape[0] > k                   # the slot went on with another game
        np.testing.assert_array_equal(bits(rows_s[g][0][:k]), bits(rows_q[g][0]), err_msg="first game of slot %d" % g)
        np.testing.assert_array_equal(bits(rows_s[g][1][:k]), bits(rows_q[g][1]), err_msg="labels of the first game of slot %d" % g)
    planes, policy, value, gidx = s.examples()
    occupied = np.abs(planes.reshape(-1, 2, 9)[:, 0]) == 1.0               # the two-plane encoder: +-1 a stone, 0.001 an empty cell
    assert occupied.any() and not occupied.all()
    assert not (policy[:, :9][occupied] != 0).any(), "a row puts weight on an occupied cell"
    assert (policy[:, 9] == 0).all()                                       # mnk has no Pass child
    assert (policy >= 0).all() and (np.abs(policy.astype(np.float64).sum(axis=1) - 1.0) <= 10 * 2.0 ** -24).all()
    for x in (s, twin, q):
        x.close()


def make_net(ctx, S, K, L):
    net = A.Net(ctx, K, L, 64, S, S, 18, S * S + 1, bn_mode=capi.BN_IDENTITY)
    net.init_random(1337)
    for i in range(net.num_params()):
        name, n = net.param_info(i)
        if name.endswith("_gamma"):
            net.set_param(i, np.ones(n, np.float32))
        elif name.endswith("_beta"):
            net.set_param(i, np.zeros(n, np.float32))
    net.commit()
    net.set_compute_mode(capi.COMPUTE_WINO_H2)
    net.set_tower_queues(2)
    return net


@pytest.mark.parametrize("mode", [1, 2])
def test_split_and_skewed_step(ctx, mode):
    """AGZ_INF_NET agents: the split step needs the chained tower of one shared net (tests/test_split_step_gpu.py's small shape, 416 games
    of 9x9 Go on a K = 256 four-block net).  It promises the joined step's examples bit for bit; both arenas record TARGET_VISITS rows,
    and a sample of the split arena's rows is checked against the host definition as well."""
    S, G, budget, tau = 9, 416, 8, 0.5
    net = make_net(ctx, S, 256, 4)
    arenas = []
    for m in (0, mode):
        a = A.Arena(ctx, capi.GAME_WQ, S, S, 0, 7.5, encoder=capi.ENC_WQ, n_games=G, seed=31, Budget=budget)
        for agent in (0, 1):
            a.set_inferencer(agent, capi.INF_NET, net)
        a.set_policy_target(VISITS, tau)
        a.reset(np.array([(i % 2) == 1 for i in range(G)], dtype=np.uint8))
        a.random_moves(np.random.default_rng(31).integers(0, 30, size=G).astype(np.int32), 31)
        a.set_split(m)
        arenas.append(a)
    joined, split = arenas
    sample = list(range(0, G, 37)) + [G // 2 - 1, G // 2, G - 1]
    for ply in range(2):
        for a in arenas:
            a.begin_move()
            a.simulate(budget)
        roots = {g: split.root_children(g, searching_agent(split, g))[:2] for g in sample}
        for a in arenas:
            a.end_move(True)
        ej, es = joined.examples(), split.examples()
        assert es[1].shape[0] == (ply + 1) * G
        oj, os_ = np.argsort(ej[3], kind="stable"), np.argsort(es[3], kind="stable")
        for x, y, name in zip(ej, es, ("planes", "policy", "value", "game")):
            np.testing.assert_array_equal(bits(x[oj]), bits(y[os_]), err_msg="ply %d: example %s" % (ply, name))
        for g in sample:
            newest = es[1][es[3] == g][-1]
            np.testing.assert_array_equal(bits(newest), bits(capi.visit_target_of(roots[g][0], roots[g][1], S * S, tau)), err_msg="ply %d game %d" % (ply, g))
    js, ss = joined.split_steps(), split.split_steps()
    assert js[0] == 0 and js[1] == 2 * budget, js
    assert ss[0] == 2 * budget and ss[1] == 0, ss
    for a in arenas:
        a.close()
    net.close()


# ---- 5. checkpoint ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_continuation(ctx, tmp_path):
    tau = 0.5
    conf = dict(RandomCount=6, RandomTemperature=1.0)
    path = str(tmp_path / "target.ckpt")
    a = make(ctx, "wq5", target=(VISITS, tau), **conf)
    for ply in range(3):
        checked_move(a, tau, "before the save, ply %d" % ply)
    a.save(path)
    saved_rows = a.stats()["examples"]
    assert saved_rows == 3 * a.n_games
    b = make(ctx, "wq5", seed=977, **conf)
    c = make(ctx, "wq5", seed=977, **conf)
    for x in (b, c):
        x.load(path)
        assert x.get_policy_target() == {"kind": REF, "temperature": 1.0}   # the setting is not in the file
    c.set_policy_target(VISITS, tau)
    for ply in range(2):
        checked_move(a, tau, "uninterrupted, ply %d" % ply)
        checked_move(c, tau, "after the load, ply %d" % ply)
        b.begin_move()
        b.simulate(b.mconf.Budget)
        b.end_move(True)
    assert_same(c, a, "2 plies after the load")
    assert_same(b, a, "the arena that did not re-apply the setting searches alike", examples=False)
    rows_a, rows_b = rows_by_game(a), rows_by_game(b)
    for g in range(a.n_games):                                          # the rows recorded before the save are ordinary example rows of the file
        np.testing.assert_array_equal(bits(rows_b[g][0][:3]), bits(rows_a[g][0][:3]), err_msg="the saved rows of game %d" % g)
    new_b = np.concatenate([rows_b[g][0][3:] for g in range(b.n_games)])
    assert new_b.shape[0] > 0 and set(np.unique(new_b).tolist()) <= {0.0, 1.0}, "without the setting the loaded arena records the reference's one-hot rows"
    for x in (a, b, c):
        x.close()


# ---- 6. downstream ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def finished_3x3(ctx):
    """8 games of mnk 3x3 played to the end under TARGET_VISITS at tau = 1: the labelled examples, on the host"""
    a = make(ctx, "mnk3", target=(VISITS, 1.0))
    a.play(0)
    planes, policy, value, gidx = a.examples()
    assert all(a.game(g)[1]["ended"] for g in range(a.n_games)) and policy.shape[0] == a.stats()["moves_played"] >= 40
    a.close()
    return planes.reshape(-1, 2, 3, 3), policy, value


def test_the_dihedral_augmenter_permutes_the_cells_and_keeps_the_pass_entry(ctx):
    a = make(ctx, "wq5", target=(VISITS, 1.0), PassPreference=capi.PREFER_PASS)
    a.play(6)
    planes, policy, value, _ = a.examples()
    a.close()
    n, S = policy.shape[0], 5
    assert 12 <= n <= 24 and (policy[:, 25] > 0).any(), "no row with a visited Pass child"
    ex = A.Examples(ctx, 18, S, S, S * S + 1)
    ex.append_host(planes, policy, value)
    ex.augment_dihedral()
    assert len(ex) == 8 * n
    _, q, v = ex.get()
    for k in range(8):
        src = capi.symmetry_map(S, k)
        np.testing.assert_array_equal(bits(q[k::8, :25]), bits(policy[:, src]), err_msg="cells under S_%d" % k)
        np.testing.assert_array_equal(bits(q[k::8, 25]), bits(policy[:, 25]), err_msg="the Pass entry under S_%d" % k)
        np.testing.assert_array_equal(bits(v[k::8]), bits(value))
    ex.close()


def test_one_alphazero_step_on_visit_rows(ctx, finished_3x3):
    planes, policy, value = finished_3x3
    B = 8
    pick = np.linspace(0, policy.shape[0] - 1, B).astype(int)            # openings, middle games and last moves
    x, pi, v = planes[pick], policy[pick], value[pick]
    assert set(np.unique(v).tolist()) <= {-1.0, 0.0, 1.0}
    p64 = pi.astype(np.float64)
    entropy = float(np.mean(-np.sum(np.where(p64 > 0, p64 * np.log(np.where(p64 > 0, p64, 1.0)), 0.0), axis=1)))
    assert 0.0 < entropy <= np.log(10.0)
    dt = A.Trainer(ctx, 32, 1, 16, 3, 3, 2, 10, B, tied=True)
    dt.init_random(3)
    dt.set_loss(capi.LOSS_ALPHAZERO)
    cost = dt.forward_backward(x, pi, v)
    pcost, vcost = dt.costs()
    print("policy term %.6f, batch-mean target entropy %.6f, value term %.6f" % (pcost, entropy, vcost))
    assert np.isfinite([cost, pcost, vcost]).all()
    assert pcost >= entropy - 1e-4                                        # cross-entropy >= entropy
    stepped = dt.batch(x, pi, v, lr=0.01)                                 # one step
    assert np.isfinite(stepped) and np.isfinite(dt.costs()).all()
    after = dt.forward_backward(x, pi, v)
    assert np.isfinite(after) and dt.costs()[0] >= entropy - 1e-4
    dt.close()
