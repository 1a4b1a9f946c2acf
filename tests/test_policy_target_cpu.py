"""CPU: root visit counts as policy targets (agogo_amd/csrc/target.hpp, DESIGN.md §2 visit-target) on the code the kernel compiles.

target.hpp is the one definition host and device share: k_end_move (engine.hip) and the host function agz_visit_target_of.  It uses only
IEEE double + - * /, integer and bit operations (ln_b / exp_b are noise.hpp's), so a pure-Python restatement (Python floats are the same
doubles, Python integers are exact) must agree with it BIT FOR BIT: tests/cpp/target_check.cpp under plain g++ at -O0 and -O2, and
agz_visit_target_of through libagz."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
PASS = -1
TAUS = (1.0, 0.5, 0.25, 2.0, 0.03)


# ---- the declared definition, restated -------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dfrom(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def ln_b(x):
    b = dbits(x)
    e = ((b >> 52) & 0x7FF) - 1023
    m = dfrom((b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    if m > 1.4142135623730951:
        m = m * 0.5
        e += 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    acc = 0.0
    for k in range(12, -1, -1):
        acc = acc * s2 + 1.0 / float(2 * k + 1)
    return float(e) * 0.6931471805599453 + (2.0 * s) * acc


def exp_b(y):
    if y < -700.0:
        return 0.0
    t = y * 1.4426950408889634 + 0.5
    k = int(t)
    if float(k) > t:
        k -= 1
    r = y - float(k) * 0.6931471805599453
    acc = 1.0
    for j in range(16, 0, -1):
        acc = 1.0 + (acc * r) / float(j)
    return acc * dfrom((k + 1023) << 52)


def weight_py(n, nmax, tau):
    """w_i as a Python integer; tau is already the double of the float the caller passes"""
    if tau == 1.0:
        return n
    if n == nmax:
        return 1 << 40
    if n == 0:
        return 0
    return int(exp_b(ln_b(float(n) / float(nmax)) / tau) * 1099511627776.0)


def row_py(moves, visits, A, tau32):
    """the row as float32; None when Nmax == 0"""
    tau = f32(tau32)
    visits = [int(v) for v in visits]
    nmax = max(visits)
    if nmax == 0:
        return None
    w = [weight_py(v, nmax, tau) for v in visits]
    S = sum(w)
    assert S < 1 << 53
    row = np.zeros(A + 1, np.float32)
    for mv, wi in zip(moves, w):
        row[A if mv == PASS else mv] = np.float32(float(wi) / float(S))      # one rounding, double -> float
    return row


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def children(A, n, with_pass, rng, kind):
    """n distinct children of an action space A (one of them Pass when with_pass) and a visit vector of the given kind"""
    cells = rng.permutation(A)[:n - (1 if with_pass else 0)].astype(np.int32)
    moves = np.concatenate([cells, np.array([PASS], np.int32)]) if with_pass else cells
    moves = moves[rng.permutation(n)]
    if kind == "budget":            # what a search leaves: a few hundred visits spread unevenly
        v = rng.integers(0, 200, n)
    elif kind == "ties":            # several children at Nmax
        v = rng.integers(0, 4, n) * 25
        v[rng.integers(0, n)] = 75
        if n > 1:
            v[(int(np.argmax(v)) + 1) % n] = 75
    elif kind == "zeros":           # mostly unvisited
        v = np.where(rng.random(n) < 0.7, 0, rng.integers(1, 50, n))
        v[rng.integers(0, n)] = 31
    else:                           # "large": N = 2^24 - 1 at the top, the rest anywhere below
        v = rng.integers(0, 1 << 24, n)
        v[rng.integers(0, n)] = (1 << 24) - 1
    return moves, v.astype(np.uint32)


# (action space, children, Pass child): n = 1; 3x3; 5x5 Go with Pass; 9x9 Go; 19x19 Go
SHAPES = ((9, 1, False), (9, 9, False), (25, 26, True), (81, 82, True), (361, 362, True))
KINDS = ("budget", "ties", "zeros", "large")


def all_cases():
    rng = np.random.default_rng(20261021)
    for A, n, wp in SHAPES:
        for kind in KINDS:
            moves, visits = children(A, n, wp, rng, kind)
            # the case holds what it is named for
            assert len(set(moves.tolist())) == n and (PASS in moves) == wp
            assert kind != "ties" or n == 1 or int((visits == visits.max()).sum()) >= 2
            assert kind != "zeros" or n <= 2 or int((visits == 0).sum()) >= 1
            assert kind != "large" or int(visits.max()) == (1 << 24) - 1
            yield A, moves, visits, kind


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
FUNCS = {"agz_arena_set_policy_target": 2, "agz_arena_get_policy_target": 2, "agz_visit_target_of": 6}


def test_the_three_functions_are_declared_exported_bound_and_called_from_go():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agz.h")).read(), flags=re.S)
    raw = C.CDLL(capi.lib_path())
    L = capi.lib()
    go = open(os.path.join(ROOT, "go", "agzhip", "agzhip.go")).read()
    for name, nargs in FUNCS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/agz.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(raw, name), "%s is not exported" % name
        assert len(getattr(L, name).argtypes) == nargs, name
        assert re.search(r"C\.%s\(" % name, go), "go/agzhip never calls %s" % name
    assert re.search(r"#define\s+AGZ_TARGET_REFERENCE\s+0\b", hdr) and re.search(r"#define\s+AGZ_TARGET_VISITS\s+1\b", hdr)
    assert re.search(r"typedef\s+struct\s+agz_target_conf\s*\{\s*int32_t\s+kind\s*;\s*float\s+temperature\s*;\s*int32_t\s+reserved\[2\]\s*;\s*\}\s*agz_target_conf\s*;", hdr)
    assert C.sizeof(capi.TargetConf) == 16
    assert [f[0] for f in capi.TargetConf._fields_] == ["kind", "temperature", "reserved"]
    assert (capi.TARGET_REFERENCE, capi.TARGET_VISITS) == (0, 1)
    for meth in ("set_policy_target", "get_policy_target"):
        assert hasattr(capi.Arena, meth), meth
    assert callable(capi.visit_target_of)
    for fn in ("func (a *BatchedArena) SetPolicyTarget(", "func VisitTargetOf("):
        assert fn in go, fn
    hpp = open(os.path.join(ROOT, "agogo_amd", "host", "agogo.hpp")).read()
    assert "SetPolicyTarget" in hpp and "int PolicyTarget = AGZ_TARGET_REFERENCE" in hpp and "float TargetTemperature = 1.f" in hpp
    # the Config fields are applied to the self-play arena only, and are not written into a SaveRun file
    assert hpp.count("sp.SetPolicyTarget(") == 1 and hpp.count(".SetPolicyTarget(") == 1
    assert '"PolicyTarget"' not in hpp and '"TargetTemperature"' not in hpp


# ---- 1. bit for bit against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_the_host_function_equals_the_python_restatement_bit_for_bit(tau):
    seen = set()
    for A, moves, visits, kind in all_cases():
        got = capi.visit_target_of(moves, visits, A, tau)
        want = row_py(moves, visits, A, tau)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg="A %d n %d %s tau %r" % (A, moves.size, kind, tau))
        seen.add((moves.size, kind))
    assert len(seen) == len(SHAPES) * len(KINDS)


# ---- 2. the header under plain g++ -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("target_check")
    outs = []
    for opt in ("-O0", "-O2"):
        exe = str(d / ("target_check" + opt))
        subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "target_check.cpp")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "TARGET OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        outs.append(out.stdout)
    assert outs[0] == outs[1], "target.hpp prints different bits at -O0 and at -O2"
    return [line.split() for line in outs[0].splitlines()]


def test_the_header_prints_the_same_bits_at_O0_and_O2_and_python_and_libagz_agree(check_lines):
    seen = {"w": 0, "row": 0}
    for w in check_lines:
        if w[0] == "w":
            tau = float(np.array([int(w[3], 16)], np.uint32).view(np.float32)[0])
            assert weight_py(int(w[1]), int(w[2]), tau) == int(w[4]), w
        elif w[0] == "row":
            A, n = int(w[1]), int(w[3])
            tau = np.array([int(w[2], 16)], np.uint32).view(np.float32)[0]
            moves = np.array([int(x) for x in w[4:4 + n]], np.int32)
            visits = np.array([int(x) for x in w[4 + n:4 + 2 * n]], np.uint32)
            got = np.array([int(x, 16) for x in w[4 + 2 * n:]], np.uint32)
            assert got.size == A + 1
            np.testing.assert_array_equal(got, bits(row_py(moves, visits, A, tau)), err_msg="A %d n %d tau %r" % (A, n, tau))
            np.testing.assert_array_equal(got, bits(capi.visit_target_of(moves, visits, A, tau)))
        else:
            continue
        seen[w[0]] += 1
    assert seen["w"] == 7 * 40 and seen["row"] == 7 * 7 * 3, seen


# ---- 3. order independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_any_order_of_the_children_gives_the_identical_row(tau):
    rng = np.random.default_rng(7)
    for A, moves, visits, kind in all_cases():
        base = bits(capi.visit_target_of(moves, visits, A, tau))
        orders = [np.arange(moves.size)[::-1], np.argsort(-visits.astype(np.int64), kind="stable"), rng.permutation(moves.size), rng.permutation(moves.size)]
        for p in orders:
            np.testing.assert_array_equal(bits(capi.visit_target_of(moves[p], visits[p], A, tau)), base, err_msg="A %d %s" % (A, kind))


# ---- 4. row content --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
def test_row_content(tau):
    for A, moves, visits, kind in all_cases():
        row = capi.visit_target_of(moves, visits, A, tau)
        assert row.shape == (A + 1,) and row.dtype == np.float32
        idx = np.where(moves == PASS, A, moves)
        absent = np.setdiff1d(np.arange(A + 1), idx)
        assert not bits(row)[absent].any(), "an entry without a child is not +0.0"
        assert (row >= 0).all()
        if PASS in moves:               # Pass lands at index A (a small weight may underflow to 0 at a low temperature, never the largest)
            v_pass = int(visits[moves == PASS][0])
            if v_pass == 0:
                assert bits(row)[A] == 0
            if v_pass == int(visits.max()):
                assert row[A] == row.max() > 0
            if tau >= 1.0:
                assert (row[A] > 0) == (v_pass > 0)
        else:
            assert bits(row)[A] == 0
        # every entry carries one float rounding of a value in [0, 1]: the float64 sum is within (A + 1) 2^-24 of 1
        total = float(row.astype(np.float64).sum())
        print("A %d n %d %s tau %g: |sum - 1| = %.3g (bound %.3g)" % (A, moves.size, kind, tau, abs(total - 1.0), (A + 1) * 2.0 ** -24))
        assert abs(total - 1.0) <= (A + 1) * 2.0 ** -24
        # the order of the entries is the order of the visits
        assert (np.diff(row[idx][np.argsort(visits, kind="stable")]) >= 0).all()
        assert (row[idx][visits == visits.max()] == row.max()).all()
        if tau == 1.0:
            want = np.zeros(A + 1, np.float32)
            want[idx] = (visits.astype(np.float64) / np.float64(visits.astype(np.float64).sum())).astype(np.float32)
            np.testing.assert_array_equal(bits(row), bits(want))


def test_a_low_temperature_sharpens_and_a_high_one_flattens():
    moves, visits = np.arange(4, dtype=np.int32), np.array([100, 50, 10, 0], np.uint32)
    r1, rs, rf = (capi.visit_target_of(moves, visits, 9, t) for t in (1.0, 0.25, 4.0))
    assert rs[0] > r1[0] > rf[0] and rs[2] < r1[2] < rf[2]
    assert rs[3] == r1[3] == rf[3] == 0.0          # an unvisited child stays at zero at every temperature
    # tau = 0.5 squares the ratios: w = (1, 1/4, 1/100) 2^40 up to the few ulp of ln_b / exp_b and the truncation
    r = capi.visit_target_of(moves, visits, 9, 0.5).astype(np.float64)
    np.testing.assert_allclose(r[:3], np.array([1.0, 0.25, 0.01]) / 1.26, rtol=1e-6)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_row_untouched():
    L = capi.lib()
    pi, pu, pf = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def call(moves, visits, n, A, tau, row_null=False, moves_null=False, visits_null=False):
        mv = np.ascontiguousarray(moves, np.int32)
        vis = np.ascontiguousarray(visits, np.uint32)
        row = np.full(4200, -7.0, np.float32)
        rc = L.agz_visit_target_of(None if moves_null else mv.ctypes.data_as(pi), None if visits_null else vis.ctypes.data_as(pu), n, A, tau,
                                   None if row_null else row.ctypes.data_as(pf))
        assert (row == -7.0).all() or rc == 0, "a refused call wrote into the row"
        return rc, row

    ok_m, ok_v = [0, 4, PASS], [3, 0, 5]
    rc, row = call(ok_m, ok_v, 3, 9, 1.0)
    assert rc == 0 and (row[:10] != -7.0).all() and (row[10:] == -7.0).all()
    assert call(ok_m, ok_v, 3, 9, 1.0, row_null=True)[0] == E_INVALID
    assert call(ok_m, ok_v, 3, 9, 1.0, moves_null=True)[0] == E_INVALID
    assert call(ok_m, ok_v, 3, 9, 1.0, visits_null=True)[0] == E_INVALID
    big_m, big_v = np.arange(4097, dtype=np.int32) % 4096, np.ones(4097, np.uint32)
    for n in (0, -1, 4097):
        assert call(big_m, big_v, n, 4096, 1.0)[0] == E_INVALID, n
    for A in (0, -1, 4097):
        assert call([0], [1], 1, A, 1.0)[0] == E_INVALID, A
    for bad in (9, 10, -2, -3, 1 << 20):                # outside [0, A) and not Pass (Resign, -2, is no child of a root)
        assert call([0, bad], [1, 1], 2, 9, 1.0)[0] == E_INVALID, bad
    assert call([3, 4, 3], [1, 1, 1], 3, 9, 1.0)[0] == E_INVALID
    assert call([PASS, 4, PASS], [1, 1, 1], 3, 9, 1.0)[0] == E_INVALID
    for tau in (0.0, -1.0, float("inf"), float("-inf"), float("nan"), -0.0):
        assert call(ok_m, ok_v, 3, 9, tau)[0] == E_INVALID, tau
    assert call(ok_m, [0, 0, 0], 3, 9, 1.0)[0] == E_INVALID
    assert call(ok_m, [0, 0, 0], 3, 9, 0.5)[0] == E_INVALID
    # the limits themselves are accepted: n = 4096 children of an action space of 4096
    rc, row = call(np.arange(4096, dtype=np.int32), np.full(4096, 0xFFFFFFFF, np.uint32), 4096, 4096, 0.5)
    assert rc == 0 and (row[:4096] == np.float32(1.0 / 4096)).all() and row[4096] == 0.0
    with pytest.raises(capi.AgzError):
        capi.visit_target_of([0, 0], [1, 2], 9, 1.0)
