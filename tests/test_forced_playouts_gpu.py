"""GPU: forced playouts and policy-target pruning at the root (agz_arena_set_forced_playouts, DESIGN.md §2 forced-playouts).

The reference has no such rule, so the references here are (a) the host functions agz_root_select_of and agz_pruned_target_of —
tests/test_forced_playouts_cpu.py ties them bit for bit to a pure-Python restatement of the declared definitions — applied to the root
children read back from the device, and (b) twin arenas from the same seed for everything that must stay bit-identical, compared with
test_policy_target_gpu.assert_same (histories, boards, both roots' moves, visits, blackScores bits and prior bits, counters, example
rows).  AGZ_INF_HASH agents.  Nothing here depends on timing."""
import ctypes as C

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_playout_cap_gpu import FAST_BUDGET, NOISE, assert_game_same, balanced_seed, slot_keys
from test_policy_target_gpu import GAMES, assert_same, bits, rows_by_game, searching_agent

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
FULL, FAST = capi.CAP_FULL, capi.CAP_FAST
REF, VISITS = capi.TARGET_REFERENCE, capi.TARGET_VISITS


def make(ctx, game, seed=5, forced=None, cap=None, noise=False, target=None, lanes=1, **over):
    """forced / cap: None (never configured) or the keyword arguments of Arena.set_forced_playouts / set_playout_cap"""
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
    if forced is not None:
        a.set_forced_playouts(**forced)
    a.reset(np.array([g % 2 for g in range(a.n_games)], np.uint8))       # both agents get to search first somewhere
    return a


def move(a, k=None, record=True):
    a.begin_move()
    a.simulate(a.mconf.Budget if k is None else k)
    a.end_move(record)


def roots_of(a):
    """game -> (player to move, (moves, visits, blackScores, priors) of the searching agent's root) for every unfinished game"""
    out = {}
    for g in range(a.n_games):
        agent = searching_agent(a, g)
        if agent is not None:
            out[g] = (a.game(g)[1]["to_move"], a.root_children(g, agent))
    return out


# ---- 1. off is untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["mnk3", "c4", "wq5", "wq9"])
def test_off_k_zero_and_fast_plies_are_the_arena_without_the_setting(ctx, game):
    budget = GAMES[game]["Budget"]
    never = make(ctx, game)
    assert never.get_forced_playouts() == {"k": 2.0, "on": False, "prune": True}      # the defaults
    arenas = [make(ctx, game, forced=dict(k=8.0, on=False)),
              make(ctx, game, forced=dict(k=0.0, on=True, prune=False))]
    for x in [never] + arenas:
        x.play(4, True)
    for i, x in enumerate(arenas):
        assert_same(x, never, "%s arena %d" % (game, i))
    assert never.stats()["examples"] > 0
    # every ply a FAST search of the whole budget: a FAST ply does not force (and records nothing) — the plain arena played unrecorded
    unrec = make(ctx, game)
    capped = make(ctx, game, forced=dict(k=2.0), cap=dict(p_full=0.0, fast_budget=budget, seed=3), target=(REF, 1.0))
    unrec.play(4, False)
    capped.play(4, True)
    assert_same(capped, unrec, "%s on, k = 2, every ply FAST" % game)
    assert_same(capped, never, "%s on, k = 2, every ply FAST, against the recorded arena" % game, examples=False)
    # visit targets with k = 0 and prune off: today's AGZ_TARGET_VISITS arena
    vplain, vzero = make(ctx, game, target=(VISITS, 1.0)), make(ctx, game, target=(VISITS, 1.0), forced=dict(k=0.0, on=True, prune=False))
    for x in (vplain, vzero):
        x.play(2, True)
    assert_same(vzero, vplain, "%s visit targets, k = 0, prune off" % game)
    for x in [never, unrec, capped, vplain, vzero] + arenas:
        x.close()


# ---- 2. every root step is the host function -------------------------------------------------------------------------------------
STEPS = [(game, k) for game in ("mnk3", "c4", "wq5") for k in (2.0, 8.0)]
FORCED_STEPS = {}                                                        # (game, k) -> (forced steps, unforced steps), filled by the cases


@pytest.mark.parametrize("game,k", STEPS, ids=["%s-k%g" % c for c in STEPS])
def test_every_root_step_is_the_host_function(ctx, game, k):
    a = make(ctx, game, forced=dict(k=k), target=(VISITS, 1.0))
    puct = a.mconf.PUCT
    n_forced = n_plain = n_null = 0
    for ply in range(3):                                                  # plies 1 and 2 search re-rooted trees with carried visits
        a.begin_move()
        before = roots_of(a)
        for step in range(a.mconf.Budget):
            nonnull = a.stats()["sims_nonnull"]
            a.simulate(1)
            after = roots_of(a)
            grown = 0
            for g, (player, (mv, vis, bs, pr)) in before.items():
                mv2, vis2, _, _ = after[g][1]
                np.testing.assert_array_equal(mv2, mv)
                delta = vis2.astype(np.int64) - vis.astype(np.int64)
                if not delta.any():                                       # a null simulation: nothing was backed up
                    n_null += 1
                    continue
                idx, forced = capi.root_select_of(vis, bs, pr, player, puct, k)
                want = np.zeros(mv.size, np.int64)
                want[idx] = 1
                np.testing.assert_array_equal(delta, want, err_msg="%s k %g ply %d step %d game %d (forced %d)" % (game, k, ply, step, g, forced))
                grown += 1
                n_forced += forced
                n_plain += not forced
            assert grown == a.stats()["sims_nonnull"] - nonnull
            before = after
        a.end_move(True)
    print("%s k %g: %d forced, %d unforced, %d null steps" % (game, k, n_forced, n_plain, n_null))
    FORCED_STEPS[(game, k)] = (n_forced, n_plain)
    assert n_plain > 0
    if k == 8.0:
        assert n_forced > 0, "no step was forced at k = 8: the rule was not exercised"
    a.close()


def test_the_k_2_cases_forced_some_step(ctx):
    """the k = 2 cases together have at least one forced step (the cases above leave their counts; run alone, this one runs them)"""
    for game, k in STEPS:
        if k == 2.0 and (game, k) not in FORCED_STEPS:
            test_every_root_step_is_the_host_function(ctx, game, k)
    counts = {c: FORCED_STEPS[c] for c in STEPS if c[1] == 2.0}
    assert sum(f for f, _ in counts.values()) > 0, counts


# ---- 3. lane rounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2.0, 8.0])
def test_lane_rounds_follow_the_host_function_with_accumulating_marks(ctx, k):
    lanes = 4
    a = make(ctx, "wq5", forced=dict(k=k), lanes=lanes)
    puct = a.mconf.PUCT
    compared = n_forced = 0
    for ply in range(2):
        a.begin_move()
        before = roots_of(a)
        for rnd in range(a.mconf.Budget // lanes):
            a.simulate(lanes)
            after = roots_of(a)
            for g, (player, (mv, vis, bs, pr)) in before.items():
                delta = after[g][1][1].astype(np.int64) - vis.astype(np.int64)
                if int(delta.sum()) != lanes:                              # a lane of this round met a null leaf: its path was not backed up
                    continue
                marks, want = np.zeros(mv.size, np.uint8), np.zeros(mv.size, np.int64)
                for lane in range(lanes):                                  # the lanes descend in order, each sees the marks of the earlier ones
                    idx, forced = capi.root_select_of(vis, bs, pr, player, puct, k, marks=marks)
                    marks[idx] = 1
                    want[idx] += 1
                    n_forced += forced
                np.testing.assert_array_equal(delta, want, err_msg="k %g ply %d round %d game %d" % (k, ply, rnd, g))
                compared += 1
            before = after
        a.end_move(True)
    print("k %g: %d rounds compared, %d forced lanes" % (k, compared, n_forced))
    assert compared >= a.n_games * 2 * (a.mconf.Budget // lanes) // 2 and n_forced > 0
    a.close()


# ---- 4. the row ------------------------------------------------------------------------------------------------------------------
def checked_move(a, k, tau, prune, what, tally):
    """one begin / simulate / end round: the newest row of every game is the host definition of the mover's root as it stood before
    end_move — agz_pruned_target_of with prune, agz_visit_target_of without"""
    a.begin_move()
    a.simulate(a.mconf.Budget)
    roots = roots_of(a)
    before = {g: r[0].shape[0] for g, r in rows_by_game(a).items()}
    a.end_move(True)
    after = rows_by_game(a)
    for g in range(a.n_games):
        grew = after[g][0].shape[0] - before[g]
        if g not in roots or roots[g][1][1].size == 0 or int(roots[g][1][1].max()) < (2 if prune else 1):
            assert grew == 0, (what, g, grew)
            continue
        assert grew == 1, "%s: game %d recorded %d rows on a searched ply" % (what, g, grew)
        player, (mv, vis, bs, pr) = roots[g]
        if prune:
            want, npl = capi.pruned_target_of(mv, vis, bs, pr, a.action_space, player, a.mconf.PUCT, k, tau)
            n_play = vis.astype(np.int64) - 1
            tally["rows"] += 1
            tally["pruned"] += bool((npl < n_play).any())
            tally["zeroed"] += bool(((npl == 0) & (n_play > 0)).any())
            tally["differs"] += bool((bits(want) != bits(capi.visit_target_of(mv, vis, a.action_space, tau))).any())
        else:
            want = capi.visit_target_of(mv, vis, a.action_space, tau)
        np.testing.assert_array_equal(bits(after[g][0][-1]), bits(want), err_msg="%s: game %d, %d children" % (what, g, mv.size))


ROWS = [(game, tau, {}) for game in ("mnk3", "c4", "wq5", "wq9") for tau in (1.0, 0.5)]
ROWS.append(("wq5", 0.5, dict(RandomCount=10, RandomTemperature=1.0)))    # randomizeChildren reorders the block in the same kernel
ROW_TALLY = {}


@pytest.mark.parametrize("game,tau,over", ROWS, ids=["%s-%g%s" % (g, t, "-random" if o else "") for g, t, o in ROWS])
def test_the_row_is_the_pruned_target_of_the_read_back_root(ctx, game, tau, over):
    k = 2.0
    a = make(ctx, game, forced=dict(k=k), target=(VISITS, tau), **over)
    assert a.get_forced_playouts() == {"k": k, "on": True, "prune": True}
    tally = dict(rows=0, pruned=0, zeroed=0, differs=0)
    for ply in range(3):
        checked_move(a, k, tau, True, "%s tau %g ply %d" % (game, tau, ply), tally)
    print("%s tau %g: %r" % (game, tau, tally))
    assert tally["rows"] == 3 * a.n_games and tally["differs"] > 0      # every game recorded on every ply; the floor of one count per child is gone
    if game == "wq9":
        assert a.root_children(0, 0)[0].size > 64                          # more than one pass of the wavefront over the children
    ROW_TALLY[(game, tau, bool(over))] = tally
    a.close()


def test_some_row_was_pruned_and_some_child_pruned_to_zero(ctx):
    """summed over the cases above (run alone, this one runs them): a row with some n' < n, and a row with a child's playouts pruned to 0"""
    for game, tau, over in ROWS:
        if (game, tau, bool(over)) not in ROW_TALLY:
            test_the_row_is_the_pruned_target_of_the_read_back_root(ctx, game, tau, over)
    assert sum(t["pruned"] for t in ROW_TALLY.values()) > 0 and sum(t["zeroed"] for t in ROW_TALLY.values()) > 0, ROW_TALLY


@pytest.mark.parametrize("game", ["mnk3", "wq5"])
def test_without_prune_the_row_is_the_visit_target_of_the_forced_search(ctx, game):
    k, tau = 8.0, 0.5
    a = make(ctx, game, forced=dict(k=k, prune=False), target=(VISITS, tau))
    plain = make(ctx, game, target=(VISITS, tau))
    for ply in range(3):
        checked_move(a, k, tau, False, "%s prune off ply %d" % (game, ply), None)
        move(plain)
    differs = any((a.root_children(g, ag)[1].tolist() != plain.root_children(g, ag)[1].tolist()) or a.history(g).tolist() != plain.history(g).tolist()
                  for g in range(a.n_games) for ag in (0, 1))
    assert differs, "forcing at k = 8 left every search as it was"
    a.close()
    plain.close()


# ---- 5. with the playout cap -----------------------------------------------------------------------------------------------------
def differs(a, b, g):
    return a.history(g).tolist() != b.history(g).tolist() or any(
        bits(x).tolist() != bits(y).tolist() for ag in (0, 1) for x, y in zip(a.root_children(g, ag), b.root_children(g, ag)))


@pytest.mark.parametrize("game,lanes,over", [("mnk3", 1, {}), ("wq5", 1, {}), ("wq5", 4, dict(Budget=30, fast=10))], ids=["mnk3", "wq5", "wq5-lanes4"])
def test_with_the_playout_cap_only_full_plies_force(ctx, game, lanes, over):
    """game g of a capped, forced arena = game g of a replica driven ply by ply with g's own decision: a FULL ply with forcing (and root
    noise, and a recorded, pruned row), a FAST ply with the setting off.  A replica that forces on every ply must differ somewhere."""
    over = dict(over)
    p, k, plies = 0.5, 8.0, 6
    fast = over.pop("fast", FAST_BUDGET[game])
    keys = slot_keys(ctx, game, **over)
    cap = dict(p_full=p, fast_budget=fast, seed=balanced_seed(keys, plies, p))
    a = make(ctx, game, forced=dict(k=k), cap=cap, noise=True, target=(VISITS, 1.0), lanes=lanes, **over)
    budget = a.mconf.Budget
    decisions = []
    for ply in range(plies):
        a.begin_move()
        decisions.append([a.playout_cap(g)[2:] if searching_agent(a, g) is not None else None for g in range(a.n_games)])
        a.simulate(budget)
        a.end_move(True)
    made = [d for row in decisions for d in row if d is not None]
    n_full = sum(d[0] == FULL for d in made)
    assert 3 * n_full >= len(made) and 3 * (len(made) - n_full) >= len(made), (n_full, len(made))
    wrong = 0
    for g in range(a.n_games):
        r = make(ctx, game, target=(VISITS, 1.0), lanes=lanes, **over)
        w = make(ctx, game, target=(VISITS, 1.0), lanes=lanes, forced=dict(k=k), **over)
        for ply in range(plies):
            d = decisions[ply][g]
            kind, b = d if d is not None else (FAST, fast)              # (game g is over: whatever the other games of the replica do)
            r.set_forced_playouts(k=k, on=(kind == FULL))
            for x in (r, w):
                x.set_root_noise(NOISE[0], NOISE[1], on=(kind == FULL))
                move(x, b, record=(kind == FULL))
        assert_game_same(a, r, g, "%s lanes %d game %d" % (game, lanes, g))
        wrong += differs(a, w, g)
        r.close()
        w.close()
    assert wrong > 0, "forcing on the FAST plies as well changed no game: the gate was not exercised"
    a.close()


# ---- 6. checkpoint continuation, validation ----------------------------------------------------------------------------------------
def test_checkpoint_continuation(ctx, tmp_path):
    game, conf, forced = "wq5", dict(RandomCount=6, RandomTemperature=1.0), dict(k=8.0)
    path = str(tmp_path / "forced.ckpt")
    a = make(ctx, game, forced=forced, noise=True, target=(VISITS, 0.5), **conf)
    for ply in range(2):
        move(a)
    a.save(path)
    b, c = make(ctx, game, seed=977, **conf), make(ctx, game, seed=977, **conf)
    for x in (b, c):
        x.load(path)
        assert x.get_forced_playouts() == {"k": 2.0, "on": False, "prune": True}      # the setting is not in the file
        x.set_root_noise(*NOISE)
        x.set_policy_target(VISITS, 0.5)
    b.set_forced_playouts(**forced)
    for ply in range(3):
        for x in (a, b, c):
            move(x)
    assert_same(b, a, "3 plies after the load")
    assert any(differs(a, c, g) for g in range(a.n_games)) or bits(a.examples()[1]).tolist() != bits(c.examples()[1]).tolist(), \
        "without the setting the loaded arena continued the same way: the continuation did not depend on it"
    for x in (a, b, c):
        x.close()


def test_validation(ctx):
    L = capi.lib()
    a = make(ctx, "mnk3")
    a.set_forced_playouts(k=4.0, prune=False)
    have = a.get_forced_playouts()
    assert have == {"k": 4.0, "on": True, "prune": False}
    nan, inf = float("nan"), float("inf")
    bad = [(2.0, 2, 1, 0), (2.0, -1, 1, 0), (2.0, 1, 2, 0), (2.0, 1, -1, 0), (2.0, 1, 1, 1), (2.0, 0, 0, -1), (-0.5, 1, 1, 0), (64.5, 1, 1, 0), (nan, 1, 1, 0),
           (inf, 1, 1, 0), (-inf, 0, 0, 0), (nan, 0, 0, 0)]
    for k, on, prune, reserved in bad:
        conf = capi.ForcedConf(k, on, prune, reserved)
        assert L.agz_arena_set_forced_playouts(a.h, C.byref(conf)) == E_INVALID, (k, on, prune, reserved)
        assert b"agz_arena_set_forced_playouts" in L.agz_last_error()
        assert a.get_forced_playouts() == have
    assert L.agz_arena_set_forced_playouts(a.h, None) == E_INVALID and a.get_forced_playouts() == have
    assert L.agz_arena_get_forced_playouts(a.h, None) == E_INVALID
    assert L.agz_arena_set_forced_playouts(None, C.byref(capi.ForcedConf(2.0, 1, 1, 0))) == E_INVALID
    for k in (0.0, 64.0):                                                  # the limits themselves
        a.set_forced_playouts(k=k)
        assert a.get_forced_playouts() == {"k": k, "on": True, "prune": True}
    have = a.get_forced_playouts()
    a.begin_move()                                                        # inside a move: AGZ_E_STATE, the setting unchanged
    assert L.agz_arena_set_forced_playouts(a.h, C.byref(capi.ForcedConf(2.0, 1, 1, 0))) == E_STATE
    assert a.get_forced_playouts() == have
    a.simulate(1)
    a.end_move(False)
    a.set_forced_playouts(k=2.0, on=False)
    assert a.get_forced_playouts() == {"k": 2.0, "on": False, "prune": True}
    with pytest.raises(capi.AgzError):
        a.set_forced_playouts(k=-1.0)
    a.close()
