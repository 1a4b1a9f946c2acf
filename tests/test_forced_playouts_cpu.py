"""CPU: forced playouts and policy-target pruning at the root (agogo_amd/csrc/forced.hpp, DESIGN.md §2 forced-playouts) on the code the
kernels compile.

forced.hpp is the one definition host and device share: select_child and k_end_move (engine.hip) and the host functions
agz_root_select_of / agz_pruned_target_of.  It uses IEEE float and double operations rounded once, integers, and one correctly rounded
float square root, so a pure-Python restatement (numpy float32 for U, Python floats for the doubles, Python integers for F) must agree
with it BIT FOR BIT: tests/cpp/forced_check.cpp under plain g++ at -O0 and -O2, and the two host functions through libagz."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from agogo_amd import capi
from test_policy_target_cpu import bits, row_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PASS = -1
BLACK, WHITE = 1, 2
F32 = np.float32
KS = (0.0, 0.5, 2.0, 8.0)
TAUS = (1.0, 0.5, 2.0)


# ---- the declared definitions, restated ------------------------------------------------------------------------------------------
def evaluate_py(bs, visits, player):
    """q as float32 arrays: B / N, for White 1 - that, each operation rounded once"""
    q = bs.astype(F32) / visits.astype(F32)
    return (F32(1.0) - q).astype(F32) if player == WHITE else q


def numerator_py(visits):
    pv = int(visits.astype(np.int64).sum())
    assert pv < 1 << 32
    return np.sqrt(F32(pv)), pv                      # IEEE: the float32 square root is correctly rounded


def U_py(q, prior, puct, num, m):
    """U(i, m) = fadd(q, fmul(fmul(PUCT, P), fdiv(num, fadd(1, (float)m)))) on float32 arrays (or scalars)"""
    den = F32(1.0) + np.asarray(m, np.uint32).astype(F32)
    return q + (F32(puct) * prior) * (num / den)


def rhs_py(k32, prior, T):
    """Python floats are the doubles of the definition"""
    return (float(F32(k32)) * float(prior)) * float(T)


def F_py(rhs):
    """the largest integer f >= 0 with float(f) * float(f) <= rhs: an estimate, then the integer fix-up"""
    if not rhs > 0.0:
        return 0
    f = math.isqrt(int(rhs))
    while f > 0 and float(f) * float(f) > rhs:
        f -= 1
    while float(f + 1) * float(f + 1) <= rhs:
        f += 1
    return f


def select_py(visits, bs, prior, marks, player, puct, k32):
    """(index, forced): Node.Select over the block with the forced rule; first maximum"""
    visits, bs, prior = np.asarray(visits, np.uint32), np.asarray(bs, F32), np.asarray(prior, F32)
    n = visits.size
    num, pv = numerator_py(visits)
    T = pv - n
    b = bs
    if marks is not None and player == WHITE:
        b = bs + np.where(np.asarray(marks) != 0, F32(3.0), F32(0.0)).astype(F32)
    usa = U_py(evaluate_py(b, visits, player), prior, puct, num, visits).astype(F32)
    forced = np.zeros(n, bool)
    if F32(k32) > 0:
        for i in range(n):
            ni = int(visits[i]) - 1
            m = ni + (1 if marks is not None and marks[i] else 0)
            forced[i] = ni >= 1 and float(m) * float(m) < rhs_py(k32, prior[i], T)
    usa = np.where(forced, F32(np.inf), usa)
    best, idx = -np.inf, -1
    for i in range(n):
        if usa[i] > best:
            best, idx = usa[i], i
    return idx, bool(idx >= 0 and forced[idx])


def pruned_py(moves, visits, bs, prior, player, puct, k32):
    """n' as a list of Python integers, by a downward SCAN (the header bisects); None when the most visited child has no playout"""
    moves, visits, bs, prior = np.asarray(moves, np.int32), np.asarray(visits, np.uint32), np.asarray(bs, F32), np.asarray(prior, F32)
    n = visits.size
    cs = min(range(n), key=lambda i: (-int(visits[i]), int(moves[i])))
    if int(visits[cs]) < 2:
        return None
    num, pv = numerator_py(visits)
    T = pv - n
    q = evaluate_py(bs, visits, player)
    ustar = U_py(q, prior, puct, num, visits)[cs]
    below = U_py(q, prior, puct, num, visits) < ustar
    out = []
    for i in range(n):
        N = int(visits[i])
        if i == cs or N == 1 or not below[i]:
            out.append(N - 1)
            continue
        lo = N - min(F_py(rhs_py(k32, prior[i], T)), N - 1)
        ms = np.arange(lo, N + 1, dtype=np.uint32)
        ok = U_py(q[i], prior[i], puct, num, ms) < ustar
        assert ok[-1] and (np.diff(ok.astype(np.int8)) >= 0).all(), "U is not monotone in m"
        Np = int(ms[int(np.argmax(ok))])
        npl = Np - 1
        out.append(0 if Np < N and npl == 1 else npl)
    return out


def pruned_row_py(moves, visits, bs, prior, A, player, puct, k32, tau32):
    npl = pruned_py(moves, visits, bs, prior, player, puct, k32)
    if npl is None:
        return None, None
    return row_py(moves, npl, A, tau32), npl


# ---- random blocks ---------------------------------------------------------------------------------------------------------------
def block(rng, n, A, kind):
    """n distinct children of an action space A (one of them Pass when n == A + 1): moves, visits in [1, 2000], score sums, priors"""
    with_pass = n == A + 1
    cells = rng.permutation(A)[:n - (1 if with_pass else 0)].astype(np.int32)
    moves = np.concatenate([cells, np.array([PASS], np.int32)]) if with_pass else cells
    moves = moves[rng.permutation(n)]
    visits = np.where(rng.random(n) < 0.25, rng.integers(1, 2001, n), rng.integers(1, 7, n)).astype(np.uint32)
    if kind == "ties" and n > 1:              # several children at the largest N: c* is the smallest move among them
        top = int(visits.max())
        visits[rng.integers(0, n, 3)] = top
    prior = (rng.random(n) ** 2 + 1e-4).astype(F32)
    if kind == "equal":
        prior[:] = 1.0
    prior = (prior / prior.sum(dtype=F32)).astype(F32)
    bs = (visits.astype(F32) * (2 * rng.random(n) - 1).astype(F32)).astype(F32)
    return moves, visits, bs, prior


def all_blocks(count, seed=20261022):
    rng = np.random.default_rng(seed)
    shapes = [(1, 9), (2, 9), (9, 9), (7, 7), (26, 25), (82, 81), (362, 361), (65, 81), (129, 361)]
    for j in range(count):
        if j < len(shapes) * 3:
            n, A = shapes[j % len(shapes)]
        else:
            A = int(rng.choice([9, 25, 81, 361]))
            n = int(rng.integers(1, A + 2))
        kind = ("plain", "ties", "equal")[j % 3]
        yield (j,) + block(rng, n, A, kind) + (A, BLACK if (j // 3) % 2 == 0 else WHITE, KS[j % 4], TAUS[(j // 4) % 3], 1.0 if j % 7 == 0 else 0.75)


N_BLOCKS = 3000


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
FUNCS = {"agz_arena_set_forced_playouts": 2, "agz_arena_get_forced_playouts": 2, "agz_root_select_of": 10, "agz_pruned_target_of": 12}


def test_the_functions_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agz.h")).read(), flags=re.S)
    raw = C.CDLL(capi.lib_path())
    L = capi.lib()
    for name, nargs in FUNCS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/agz.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(raw, name), "%s is not exported" % name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert re.search(r"typedef\s+struct\s+agz_forced_conf\s*\{\s*float\s+k\s*;\s*int32_t\s+on\s*;\s*int32_t\s+prune\s*;\s*int32_t\s+reserved\s*;\s*\}\s*agz_forced_conf\s*;", hdr)
    assert C.sizeof(capi.ForcedConf) == 16
    assert [f[0] for f in capi.ForcedConf._fields_] == ["k", "on", "prune", "reserved"]
    assert [capi.ForcedConf.k.offset, capi.ForcedConf.on.offset, capi.ForcedConf.prune.offset, capi.ForcedConf.reserved.offset] == [0, 4, 8, 12]
    for meth in ("set_forced_playouts", "get_forced_playouts"):
        assert hasattr(capi.Arena, meth), meth
    assert callable(capi.root_select_of) and callable(capi.pruned_target_of)
    go = open(os.path.join(ROOT, "go", "agzhip", "agzhip.go")).read()
    assert "func (a *BatchedArena) SetForcedPlayouts(" in go and re.search(r"C\.agz_arena_set_forced_playouts\(", go)
    hpp = open(os.path.join(ROOT, "agogo_amd", "host", "agogo.hpp")).read()
    assert "SetForcedPlayouts" in hpp and "float ForcedPlayoutsK = 0.f" in hpp and "bool ForcedPrune = true" in hpp
    # the Config fields are applied to the self-play arena only, and are not written into a SaveRun file
    assert hpp.count("sp.SetForcedPlayouts(") == 1 and hpp.count(".SetForcedPlayouts(") == 1
    assert '"ForcedPlayoutsK"' not in hpp and '"ForcedPrune"' not in hpp


# ---- 1. bit for bit against the restatement --------------------------------------------------------------------------------------
def test_the_host_functions_equal_the_python_restatement_bit_for_bit():
    seen_n, forced_hits, pruned_rows, zeroed_rows, tie_stars = set(), 0, 0, 0, 0
    for j, moves, visits, bs, prior, A, player, k, tau, puct in all_blocks(N_BLOCKS):
        n = moves.size
        seen_n.add(n)
        marks = (np.random.default_rng(j).random(n) < 0.2).astype(np.uint8)
        for mk in (None, marks):
            got = capi.root_select_of(visits, bs, prior, player, puct, k, marks=mk)
            want = select_py(visits, bs, prior, mk, player, puct, k)
            assert got == want, (j, n, k, mk is not None, got, want)
            forced_hits += got[1]
            assert k > 0 or not got[1]
        want_row, want_np = pruned_row_py(moves, visits, bs, prior, A, player, puct, k, tau)
        if want_row is None:
            with pytest.raises(capi.AgzError):
                capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, k, tau)
            continue
        row, npl = capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, k, tau)
        assert npl.tolist() == want_np, (j, n, k)
        np.testing.assert_array_equal(bits(row), bits(want_row), err_msg="block %d n %d k %r tau %r" % (j, n, k, tau))
        n_play = visits.astype(np.int64) - 1
        pruned_rows += bool((npl < n_play).any())
        zeroed_rows += bool(((npl == 0) & (n_play > 0)).any())
        tie_stars += int((visits == visits.max()).sum() > 1)
    # the blocks hold what they are meant to: every width class, forced picks, pruning, pruning to zero, ties at the top
    assert {1, 2, 362} <= seen_n and len(seen_n) > 100, sorted(seen_n)
    print("forced picks %d, rows with pruning %d, with a child pruned to 0: %d, ties at the top %d" % (forced_hits, pruned_rows, zeroed_rows, tie_stars))
    assert forced_hits > 100 and pruned_rows > 100 and zeroed_rows > 100 and tie_stars > 100


# ---- 2. the header under plain g++ -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("forced_check")
    outs = []
    for opt in ("-O0", "-O2"):
        exe = str(d / ("forced_check" + opt))
        subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "forced_check.cpp")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "FORCED OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        outs.append(out.stdout)
    assert outs[0] == outs[1], "forced.hpp prints different bits at -O0 and at -O2"
    return [line.split() for line in outs[0].splitlines()]


def f32_of(hexes):
    return np.array([int(x, 16) for x in hexes], np.uint32).view(F32)


def test_the_header_prints_the_same_bits_at_O0_and_O2_and_python_and_libagz_agree(check_lines):
    seen = {"sel": 0, "prn": 0}
    forced_hits = pruned = 0
    for w in check_lines:
        if w[0] == "sel":
            player, puct, k, has_marks, n = int(w[1]), f32_of(w[2:3])[0], f32_of(w[3:4])[0], int(w[4]), int(w[5])
            p = 6
            visits = np.array([int(x) for x in w[p:p + n]], np.uint32)
            bs, prior = f32_of(w[p + n:p + 2 * n]), f32_of(w[p + 2 * n:p + 3 * n])
            marks = np.array([int(x) for x in w[p + 3 * n:p + 4 * n]], np.uint8) if has_marks else None
            got = (int(w[p + 4 * n]), bool(int(w[p + 4 * n + 1])))
            assert got == select_py(visits, bs, prior, marks, player, puct, k), w[:6]
            assert got == capi.root_select_of(visits, bs, prior, player, puct, k, marks=marks), w[:6]
            forced_hits += got[1]
        elif w[0] == "prn":
            A, player, puct, k, tau, n = int(w[1]), int(w[2]), f32_of(w[3:4])[0], f32_of(w[4:5])[0], f32_of(w[5:6])[0], int(w[6])
            p = 7
            moves = np.array([int(x) for x in w[p:p + n]], np.int32)
            visits = np.array([int(x) for x in w[p + n:p + 2 * n]], np.uint32)
            bs, prior = f32_of(w[p + 2 * n:p + 3 * n]), f32_of(w[p + 3 * n:p + 4 * n])
            npl = [int(x) for x in w[p + 4 * n:p + 5 * n]]
            row = np.array([int(x, 16) for x in w[p + 5 * n:]], np.uint32)
            assert row.size == A + 1
            want_row, want_np = pruned_row_py(moves, visits, bs, prior, A, player, puct, k, tau)
            assert npl == want_np, w[:7]
            np.testing.assert_array_equal(row, bits(want_row))
            lib_row, lib_np = capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, k, tau)
            assert lib_np.tolist() == npl
            np.testing.assert_array_equal(row, bits(lib_row))
            pruned += any(a < int(v) - 1 for a, v in zip(npl, visits))
        else:
            continue
        seen[w[0]] += 1
    assert seen["sel"] == 7 * 12 * 2 and seen["prn"] >= 7 * 12 - 12, seen      # (a block of one child with one visit has no row)
    assert forced_hits > 0 and pruned > 0


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------
def test_properties_of_the_pruned_playouts_and_the_row():
    rng = np.random.default_rng(5)
    checked = 0
    for j, moves, visits, bs, prior, A, player, k, tau, puct in all_blocks(400, seed=77):
        if int(visits.max()) < 2:
            continue
        n_play = visits.astype(np.int64) - 1
        row, npl = capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, k, tau)
        assert (npl <= n_play).all()
        cs = min(range(moves.size), key=lambda i: (-int(visits[i]), int(moves[i])))
        assert int(npl[cs]) == int(n_play[cs]) == int(n_play.max())
        # the row is the visit-target definition applied to n'
        np.testing.assert_array_equal(bits(row), bits(capi.visit_target_of(moves, npl, A, tau)))
        # k = 0: nothing can be subtracted, only the one visit of creation is removed
        row0, np0 = capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, 0.0, tau)
        assert np0.tolist() == n_play.tolist()
        np.testing.assert_array_equal(bits(row0), bits(capi.visit_target_of(moves, n_play.astype(np.uint32), A, tau)))
        # a larger k never keeps more
        assert (capi.pruned_target_of(moves, visits, bs, prior, A, player, puct, 64.0, tau)[1] <= npl).all()
        # any order of the block gives the same row and the same n' per move
        for p in (np.arange(moves.size)[::-1], rng.permutation(moves.size)):
            rowp, npp = capi.pruned_target_of(moves[p], visits[p], bs[p], prior[p], A, player, puct, k, tau)
            np.testing.assert_array_equal(bits(rowp), bits(row))
            assert npp.tolist() == npl[p].tolist()
        checked += 1
    assert checked > 350


def test_k_zero_without_marks_is_plain_node_select():
    """a direct restatement of select_child (engine.hip): usa = fadd(q, fmul(fmul(PUCT, P), fdiv(sqrt(pv), fadd(1, N)))), first maximum"""
    for j, moves, visits, bs, prior, A, player, k, tau, puct in all_blocks(600, seed=99):
        pv = F32(int(visits.astype(np.int64).sum()))
        q = bs / visits.astype(F32)
        if player == WHITE:
            q = F32(1.0) - q
        usa = q + (F32(puct) * prior) * (np.sqrt(pv) / (F32(1.0) + visits.astype(F32)))
        assert usa.dtype == F32
        assert capi.root_select_of(visits, bs, prior, player, puct, 0.0) == (int(np.argmax(usa)), False)


def test_a_forced_child_is_the_lowest_index_one_and_the_rule_is_the_declared_inequality():
    # T = 100 playouts below the root, k = 2, P = 0.1: rhs = 20 -> forced while n^2 < 20, that is n in 1..4 (never n = 0)
    visits = np.array([96, 1, 2, 5, 6], np.uint32)               # n = 95, 0, 1, 4, 5; T = 105
    visits[0] = 91                                                 # T = 90 + 0 + 1 + 4 + 5 = 100
    prior = np.array([0.6, 0.1, 0.1, 0.1, 0.1], F32)
    bs = np.array([80.0, 0.0, 0.0, 0.0, 0.0], F32)                 # Black: child 0 has by far the best value
    assert capi.root_select_of(visits, bs, prior, BLACK, 0.75, 0.0) == (0, False)
    assert capi.root_select_of(visits, bs, prior, BLACK, 0.75, 2.0) == (2, True)       # children 2 and 3 are forced: the lower index
    v2 = visits.copy()
    v2[2] = 6                                                                           # n = 5: 25 >= rhs (now 2 * 0.1f * 104)
    assert capi.root_select_of(v2, bs, prior, BLACK, 0.75, 2.0) == (3, True)
    marks = np.array([0, 0, 0, 1, 0], np.uint8)                    # a mark counts as one more playout: (4 + 1)^2 = 25 >= 20.8
    assert capi.root_select_of(v2, bs, prior, BLACK, 0.75, 2.0, marks=marks) == (0, False)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched():
    L = capi.lib()
    pi, pu, pf, pu8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)

    def prn(moves, visits, n, A, player=BLACK, puct=0.75, k=2.0, tau=1.0, null=None, bs=None, pr=None):
        mv, vis = np.ascontiguousarray(moves, np.int32), np.ascontiguousarray(visits, np.uint32)
        b = np.ascontiguousarray(bs if bs is not None else np.zeros(vis.size), F32)
        p = np.ascontiguousarray(pr if pr is not None else np.full(vis.size, 0.1), F32)
        row, npl = np.full(4200, -7.0, F32), np.full(4200, 0xABCD, np.uint32)
        rc = L.agz_pruned_target_of(None if null == "moves" else mv.ctypes.data_as(pi), None if null == "visits" else vis.ctypes.data_as(pu),
                                    None if null == "bs" else b.ctypes.data_as(pf), None if null == "pr" else p.ctypes.data_as(pf), n, A, player, puct, k, tau,
                                    None if null == "np" else npl.ctypes.data_as(pu), None if null == "row" else row.ctypes.data_as(pf))
        assert rc == 0 or ((row == -7.0).all() and (npl == 0xABCD).all()), "a refused call wrote into its outputs"
        return rc

    ok_m, ok_v = [0, 4, PASS], [3, 1, 5]
    assert prn(ok_m, ok_v, 3, 9) == 0 and prn(ok_m, ok_v, 3, 9, null="np") == 0
    for null in ("moves", "visits", "bs", "pr", "row"):
        assert prn(ok_m, ok_v, 3, 9, null=null) == E_INVALID, null
    big_m, big_v = np.arange(4097, dtype=np.int32) % 4096, np.full(4097, 2, np.uint32)
    for n in (0, -1, 4097):
        assert prn(big_m, big_v, n, 4096) == E_INVALID, n
    for A in (0, -1, 4097):
        assert prn([0], [2], 1, A) == E_INVALID, A
    for bad in (9, 10, -2, 1 << 20):
        assert prn([0, bad], [2, 2], 2, 9) == E_INVALID, bad
    assert prn([3, 4, 3], [2, 2, 2], 3, 9) == E_INVALID
    assert prn(ok_m, [3, 0, 5], 3, 9) == E_INVALID                               # a child has at least its one visit of creation
    assert prn(ok_m, [1, 1, 1], 3, 9) == E_INVALID                               # the most visited child has no playout: no row
    assert prn(ok_m, [0xFFFFFFFF, 1, 5], 3, 9) == E_INVALID                      # the sum does not fit the kernel's uint32
    for player in (0, 3, -1):
        assert prn(ok_m, ok_v, 3, 9, player=player) == E_INVALID, player
    for puct in (0.0, -0.5, 1.5, float("nan")):
        assert prn(ok_m, ok_v, 3, 9, puct=puct) == E_INVALID, puct
    for k in (-0.5, 64.5, float("inf"), float("nan")):
        assert prn(ok_m, ok_v, 3, 9, k=k) == E_INVALID, k
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        assert prn(ok_m, ok_v, 3, 9, tau=tau) == E_INVALID, tau
    assert prn(np.arange(4096, dtype=np.int32), np.full(4096, 2, np.uint32), 4096, 4096, k=64.0) == 0      # the limits themselves

    def sel(visits, n, player=BLACK, puct=0.75, k=2.0, null=None):
        vis = np.ascontiguousarray(visits, np.uint32)
        b, p = np.zeros(vis.size, F32), np.full(vis.size, 0.1, F32)
        idx, forced = C.c_int(-77), C.c_int(-77)
        rc = L.agz_root_select_of(None if null == "visits" else vis.ctypes.data_as(pu), None if null == "bs" else b.ctypes.data_as(pf),
                                  None if null == "pr" else p.ctypes.data_as(pf), None, n, player, puct, k, None if null == "index" else C.byref(idx),
                                  None if null == "forced" else C.byref(forced))
        assert rc == 0 or (idx.value == -77 and forced.value == -77), "a refused call wrote into its outputs"
        return rc

    assert sel(ok_v, 3) == 0
    for null in ("visits", "bs", "pr", "index", "forced"):
        assert sel(ok_v, 3, null=null) == E_INVALID, null
    for n in (0, -1, 4097):
        assert sel(big_v, n) == E_INVALID, n
    assert sel([3, 0, 5], 3) == E_INVALID and sel([0xFFFFFFFF, 1], 2) == E_INVALID
    assert sel(ok_v, 3, player=0) == E_INVALID and sel(ok_v, 3, puct=0.0) == E_INVALID and sel(ok_v, 3, k=-1.0) == E_INVALID and sel(ok_v, 3, k=65.0) == E_INVALID
