"""CPU: the Dirichlet root noise (agogo_amd/csrc/noise.hpp, DESIGN.md §2 root-noise) on the code the kernel compiles.

noise.hpp is the one definition host and device share: k_root_noise (engine.hip) and the host function agz_root_noise_of.  It uses only
IEEE double + - * /, integer and bit operations, so a pure-Python restatement (Python floats are the same doubles) must agree with it
BIT FOR BIT: tests/cpp/noise_check.cpp under plain g++ at -O0 and -O2, and agz_root_noise_of through libagz.  math.log / math.exp
guard the two polynomials against a mistyped constant, numpy's Generator.dirichlet is the reference for the distribution."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
E_INVALID = -1
CASES = ((1, 0.3), (2, 0.9), (10, 0.3), (26, 0.3), (82, 0.15), (362, 0.03), (5, 1.0))


# ---- the declared definition, restated -------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dfrom(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


class SplitMix64:
    def __init__(self, state):
        self.s = state & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


def u01(z):
    return (float(z >> 12) + 0.5) * 2.0 ** -52


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


def gamma_of(key, i, alpha):
    rng = SplitMix64(key + (i + 1) * 0xD1B54A32D192ED03)
    if alpha == 1.0:
        return -ln_b(u01(rng.next()))
    b = 1.0 + alpha / 2.718281828459045
    for _ in range(64):
        u1 = u01(rng.next())
        u2 = u01(rng.next())
        p = b * u1
        if p <= 1.0:
            x = exp_b(ln_b(p) / alpha)
            if u2 <= exp_b(-x):
                return x
        else:
            x = -ln_b((b - p) / alpha)
            if u2 <= exp_b((alpha - 1.0) * ln_b(x)):
                return x
    return 0.0


def eta_py(key, n, alpha32):
    """eta of one draw as float32 bits; alpha32 is the float the caller passes, widened to double"""
    alpha = f32(alpha32)
    g = [gamma_of(key, i, alpha) for i in range(n)]
    S = 0.0
    for x in g:
        S = S + x
    if S == 0.0:
        return np.full(n, np.float32(1.0 / n), np.float32)
    return np.array([x / S for x in g], np.float64).astype(np.float32)      # one rounding, double -> float


def mix_py(eps, prior, eta):
    eps, prior, eta = np.float32(eps), np.float32(prior), np.float32(eta)
    return np.float32(np.float32(np.float32(1.0) - eps) * prior) + np.float32(eps * eta)


def keys_of(seed, count):
    rng = SplitMix64(seed)
    return [rng.next() for _ in range(count)]


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
FUNCS = {"agz_arena_set_root_noise": 2, "agz_arena_get_root_noise": 2, "agz_arena_root_noise": 8, "agz_mcts_set_root_noise": 2,
         "agz_mcts_root_noise": 6, "agz_root_noise_of": 4}


def test_the_six_functions_are_declared_exported_bound_and_called_from_go():
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
        calls = [c for c in re.finditer(r"C\.%s\(" % name, go)]
        assert calls, "go/agzhip never calls %s" % name
        for c in calls:
            i, depth = c.end(), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(go[i], 0)
                i += 1
            args, d, cnt = go[c.end():i - 1], 0, 1
            for ch in args:
                d += {"(": 1, ")": -1, "[": 1, "]": -1}.get(ch, 0)
                cnt += ch == "," and d == 0
            assert cnt == nargs, (name, args)
    assert re.search(r"typedef\s+struct\s+agz_noise_conf\s*\{\s*float\s+eps\s*,\s*alpha\s*;\s*int32_t\s+on\s*,\s*reserved\s*;\s*\}\s*agz_noise_conf\s*;", hdr)
    assert C.sizeof(capi.NoiseConf) == 16
    assert [f[0] for f in capi.NoiseConf._fields_] == ["eps", "alpha", "on", "reserved"]
    for meth in ("set_root_noise", "get_root_noise", "root_noise"):
        assert hasattr(capi.Arena, meth), meth
    for meth in ("set_root_noise", "root_noise"):
        assert hasattr(capi.Mcts, meth), meth
    for fn in ("func (a *BatchedArena) SetRootNoise(", "func (a *BatchedArena) RootNoise(", "func (t *MCTS) SetRootNoise(",
               "func (t *MCTS) RootNoise(", "func RootNoiseOf("):
        assert fn in go, fn
    hpp = open(os.path.join(ROOT, "agogo_amd", "host", "agogo.hpp")).read()
    assert "SetRootNoise" in hpp and "RootNoiseEps" in hpp and "RootNoiseAlpha" in hpp


# ---- the header under plain g++ --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_check")
    outs = []
    for opt in ("-O0", "-O2"):
        exe = str(d / ("noise_check" + opt))
        subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "noise_check.cpp")])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "NOISE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        outs.append(out.stdout)
    assert outs[0] == outs[1], "noise.hpp prints different bits at -O0 and at -O2"
    return [line.split() for line in outs[0].splitlines()]


def test_the_header_prints_the_same_bits_at_O0_and_O2_and_python_agrees(check_lines):
    seen = {"ln": 0, "exp": 0, "eta": 0, "mix": 0}
    for w in check_lines:
        if w[0] == "ln":
            assert dbits(ln_b(dfrom(int(w[1], 16)))) == int(w[2], 16), w
        elif w[0] == "exp":
            assert dbits(exp_b(dfrom(int(w[1], 16)))) == int(w[2], 16), w
        elif w[0] == "eta":
            key, n = int(w[1]), int(w[2])
            alpha = np.array([int(w[3], 16)], np.uint32).view(np.float32)[0]
            want = eta_py(key, n, alpha).view(np.uint32)
            got = np.array([int(x, 16) for x in w[4:]], np.uint32)
            np.testing.assert_array_equal(got, want, err_msg="key %d n %d alpha %r" % (key, n, alpha))
        elif w[0] == "mix":
            e, p, h, r = (np.array([int(x, 16)], np.uint32).view(np.float32)[0] for x in w[1:5])
            assert mix_py(e, p, h).view(np.uint32) == r.view(np.uint32), w
        else:
            continue
        seen[w[0]] += 1
    assert seen == {"ln": 200, "exp": 200, "eta": 48, "mix": 64}, seen


# ---- the host function against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,alpha", CASES)
def test_root_noise_of_equals_the_python_restatement_bit_for_bit(n, alpha):
    for key in keys_of(1000 * n + 7, 50):
        got = capi.root_noise_of(key, n, alpha)
        assert got.dtype == np.float32 and got.shape == (n,)
        np.testing.assert_array_equal(got.view(np.uint32), eta_py(key, n, np.float32(alpha)).view(np.uint32), err_msg="key %d" % key)


def test_ln_b_and_exp_b_against_libm():
    """math.log / math.exp are the reference for the two polynomials: a guard against a mistyped constant, not a precision claim.
    Measured maxima over these 20000 points each: ln_b 2.2e-16 relative, exp_b 8.0e-14 relative (the k ln 2 product is rounded once:
    |y| ulps at y = -700); the bounds are ten times that."""
    ys = np.linspace(-700.0, 5.0, 20000)
    worst_ln = worst_exp = 0.0
    for y in ys:
        y = float(y)
        e = math.exp(y)
        worst_exp = max(worst_exp, abs(exp_b(y) - e) / e)
        x = e if y != 0.0 else 1.5
        lx = math.log(x)
        if lx != 0.0:
            worst_ln = max(worst_ln, abs(ln_b(x) - lx) / abs(lx))
    print("max relative error: ln_b %.3g, exp_b %.3g" % (worst_ln, worst_exp))
    assert worst_ln <= 2.2e-15, worst_ln
    assert worst_exp <= 8.0e-13, worst_exp
    assert exp_b(-700.5) == 0.0 and exp_b(-0.0) == 1.0 and ln_b(1.0) == 0.0


def ks_two_sample(a, b):
    a, b = np.sort(a), np.sort(b)
    allv = np.concatenate([a, b])
    fa = np.searchsorted(a, allv, side="right") / a.size
    fb = np.searchsorted(b, allv, side="right") / b.size
    return float(np.abs(fa - fb).max())


@pytest.mark.parametrize("n,alpha,N", [(10, 0.3, 20000), (5, 1.0, 20000), (362, 0.03, 600)])
def test_the_distribution_against_numpy_dirichlet(n, alpha, N):
    keys = keys_of(77 + n, N)
    assert len(set(keys)) == N
    X = np.stack([capi.root_noise_of(k, n, alpha) for k in keys])               # float32 [N, n]
    Xd = X.astype(np.float64)
    # row sums
    assert np.abs(Xd.sum(axis=1) - 1.0).max() <= n * 2.0 ** -24
    # means: every column within 6 standard errors of 1/n
    var = (1.0 / n) * (1.0 - 1.0 / n) / (n * alpha + 1.0)
    se = math.sqrt(var / N)
    dev = np.abs(Xd.mean(axis=0) - 1.0 / n).max() / se
    # variance: the mean column variance within 5 % of the analytic one
    vrel = abs(Xd.var(axis=0).mean() / var - 1.0)
    # Kolmogorov-Smirnov, column 0 against numpy's sampler, both as float32; p = 1e-6 critical value
    ref = np.random.default_rng(12345).dirichlet(np.full(n, f32(np.float32(alpha))), size=N)[:, 0].astype(np.float32)
    dks = ks_two_sample(X[:, 0], ref)
    crit = 2.69 * math.sqrt(2.0 / N)
    print("n %d alpha %g N %d: mean dev %.2f se, variance off %.3f %%, KS %.4f (critical %.4f)" % (n, alpha, N, dev, 100 * vrel, dks, crit))
    assert dev <= 6.0, dev
    assert vrel <= 0.05, vrel
    assert dks < crit, (dks, crit)


def test_root_noise_of_refuses_what_it_must_and_the_single_child():
    L = capi.lib()
    eta = np.zeros(4096, np.float32)
    p = eta.ctypes.data_as(C.POINTER(C.c_float))
    assert L.agz_root_noise_of(1, 4, 0.3, p) == 0
    for n in (0, -1, 4097):
        assert L.agz_root_noise_of(1, n, 0.3, p) == E_INVALID, n
    assert L.agz_root_noise_of(1, 4096, 0.3, p) == 0
    for alpha in (0.0, -0.3, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert L.agz_root_noise_of(1, 4, alpha, p) == E_INVALID, alpha
    assert L.agz_root_noise_of(1, 4, 0.3, None) == E_INVALID
    assert b"agz_root_noise_of" in L.agz_last_error()
    with pytest.raises(capi.AgzError, match="agz_root_noise_of"):
        capi.root_noise_of(1, 0, 0.3)
    for key in keys_of(5, 20):
        for alpha in (0.03, 0.3, 1.0):
            one = capi.root_noise_of(key, 1, alpha)
            assert one.view(np.uint32)[0] == np.float32(1.0).view(np.uint32)
    # a different key gives a different draw, the same key the same
    a, b, c = capi.root_noise_of(11, 10, 0.3), capi.root_noise_of(12, 10, 0.3), capi.root_noise_of(11, 10, 0.3)
    assert not np.array_equal(a, b) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
