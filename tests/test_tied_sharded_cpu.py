"""CPU: the tied sharded trainer's ABI (agz_trainer_create_sharded_tied) and the reference of its GPU tests.

The handle computes what agz_trainer_create_tied computes at BatchSize = n * B (include/agz.h, DESIGN §2 `tied-affine`): the gradient of a
tied tensor is built from ONE double partial per rank — over the rank's own B rows, fp32 per-row terms accumulated in double (the tower's
gamma / beta: four interleaved row slices, each in row order, the slices added in slice order; the head gamma / beta and the FC biases: the
rows in row order), not rounded — and the n partials are added in rank order in double, starting from rank 0's, and rounded once.
`oracle_tied_ranks` states exactly that in numpy over the oracle's per-row gradients (the tiled oracle of test_tied_cpu.oracle_tied, ONE
oracle run for both), and the last test checks that on the shapes and rank counts of test_tied_sharded_gpu.py it is oracle_tied's plain row
sum to within one float ulp of each element: the order the ranks add in is a matter of the last bit only.  The GPU tests import it."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import oracle_lib as O
import test_go_shim_signatures_cpu as shim_sigs
from agogo_amd import capi
from test_tied_cpu import LICENCE_CASE, batch_data, draw_tied, is_batch_shaped, oracle_tied

NAME = "agz_trainer_create_sharded_tied"
TB_RS = 4   # row slices of k_bn_bwd1_tied (train.hip)

# K, L, FC, W, H, F, A, GLOBAL B
S1 = (32, 2, 64, 5, 5, 2, 26, 6)        # HW = 25 > 24: two runs of k_bn_tied_sums; layer 0 has C = 32, half a 64-channel chunk; n = 3: 2 rows < 4 slices
S2 = (40, 2, 24, 5, 4, 3, 21, 6)        # padded channels (40 -> 64)
S3 = (32, 2, 24, 3, 3, 2, 10, 6)        # 54 rows: a step is reproducible to the bit
S3_WINO = (64, 2, 24, 3, 3, 2, 10, 6)   # ... its K = 64 variant for AGZ_COMPUTE_WINO_H2
S4 = (256, 1, 32, 19, 19, 18, 362, 4)   # the headline width
GRADIENT_CASES = [(S1, 2, "f32"), (S1, 3, "f32"), (S2, 2, "f32"), (S2, 3, "f32"), (S4, 2, "wino_h2")]


def is_tower(name):
    """gamma / beta of the tower's BatchNorms (k_bn_bwd1_tied: row slices); the other tied tensors are summed row by row (k_rows_sum)"""
    return name.endswith(("_gamma", "_beta")) and not name.startswith(("PolicyHead", "ValueHead"))


def rank_partial(rows, sliced):
    """one rank's double partial of a tied tensor from its rows' float32 terms [B_local, n]: started from -0.0 (the identity of IEEE addition)"""
    rows = rows.astype(np.float64)
    if not sliced:
        s = np.full(rows.shape[1], -0.0)
        for b in range(rows.shape[0]):
            s = s + rows[b]
        return s
    parts = []
    for k in range(TB_RS):
        s = np.full(rows.shape[1], -0.0)
        for b in range(k, rows.shape[0], TB_RS):
            s = s + rows[b]
        parts.append(s)
    s = parts[0]
    for k in range(1, TB_RS):
        s = s + parts[k]
    return s


def ranked_sum(name, g_rows, n):
    """the declared definition: g_rows [B_global, elems] float32 per-row gradients -> float32 tied gradient over n ranks"""
    B = g_rows.shape[0]
    assert B % n == 0
    Bl = B // n
    s = rank_partial(g_rows[:Bl], is_tower(name))
    for r in range(1, n):
        s = s + rank_partial(g_rows[r * Bl:(r + 1) * Bl], is_tower(name))
    return s.astype(np.float32)


def oracle_tied_ranks(case, names, P, x, pi, v, ranks):
    """ONE run of the oracle with the tied tensor in every row of its batch-shaped tensors at the global batch.  Returns
    (cost, row sums in float64 = test_tied_cpu.oracle_tied's gradients, {n: the declared rank-ordered gradients, float32} for n in ranks)"""
    K, L, FC, W, H, F, Aspace, B = case
    ot = O.TrainNet(K, L, FC, W, H, F, Aspace, B)
    for i, (nm, p) in enumerate(zip(names, P)):
        ot.set_param(i, np.tile(p, B) if is_batch_shaped(nm) else p)
    cost = ot.batch(x, pi, v, lr=0.0)
    G, R = [], {n: [] for n in ranks}
    for i, nm in enumerate(names):
        g = ot.get_grad(i)
        if not is_batch_shaped(nm):
            G.append(g.astype(np.float64))
            for n in ranks:
                R[n].append(g.copy())
            continue
        rows = g.reshape(B, -1)
        G.append(rows.astype(np.float64).sum(axis=0))
        for n in ranks:
            R[n].append(ranked_sum(nm, rows, n))
    return cost, G, R


def test_the_function_is_declared_exported_bound_and_in_the_go_shim():
    protos = shim_sigs._c_prototypes()
    assert protos.get(NAME) == 3, protos.get(NAME)
    fn = getattr(capi.lib(), NAME)                       # AttributeError if libagz.so does not export it
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 3, (fn.restype, fn.argtypes)
    assert "tied" in inspect.signature(capi.Trainer.sharded).parameters
    shim = open(shim_sigs.SHIM).read()
    m = re.search(r"^func NewShardedTrainerTied\(comm \*Comm, conf dual\.Config\) \(\*Trainer, error\) \{(.*?)^\}", shim, re.M | re.S)
    assert m, "go/agzhip has no NewShardedTrainerTied(comm, conf)"
    assert (NAME, 3) in {(name, nargs) for name, nargs, _ in shim_sigs._go_calls(m.group(1))}, "NewShardedTrainerTied does not call " + NAME


def test_create_without_a_communicator_fails_loudly():
    lib = capi.lib()
    conf = capi.NetConf(32, 1, 16, 4, 3, 3, 2, 10, 0, 1e-5)
    h = C.c_void_p()
    assert lib.agz_trainer_create_sharded_tied(None, C.byref(conf), C.byref(h)) == -1      # AGZ_E_INVALID: no communicator, no trainer
    assert not h.value and b"agz_trainer_create_sharded_tied" in lib.agz_last_error()


def test_one_rank_of_one_row_is_that_row_with_its_sign_of_zero():
    g = np.array([[0.0, -0.0, 1.5, -2.0]], np.float32)
    for name in ("L1_0_gamma", "Policy_b"):
        assert ranked_sum(name, g, 1).tobytes() == g[0].tobytes(), name
    # three ranks of two rows: slices 2 and 3 of every rank are empty and add nothing; the tower's order equals the row order here
    g = np.random.default_rng(0).normal(size=(6, 5)).astype(np.float32)
    want = ((g[0].astype(np.float64) + g[1]) + (g[2].astype(np.float64) + g[3]) + (g[4].astype(np.float64) + g[5])).astype(np.float32)
    assert ranked_sum("Init_beta", g, 3).tobytes() == want.tobytes() == ranked_sum("Value_b", g, 3).tobytes()


def test_the_row_sums_of_oracle_tied_ranks_are_oracle_tieds():
    """oracle_tied_ranks restates test_tied_cpu.oracle_tied's row sum (one oracle run serves both references): the two must stay one thing"""
    case = LICENCE_CASE
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B)
    cost, G, _ = oracle_tied_ranks(case, names, P, x, pi, v, (1, 2))
    cost_t, GT = oracle_tied(case, names, P, x, pi, v)
    assert cost == cost_t
    for nm, g, gt in zip(names, G, GT):
        assert g.dtype == gt.dtype and g.tobytes() == gt.tobytes(), nm


@pytest.mark.parametrize("case", [S1, S2, S4], ids=["S1", "S2", "S4"])
def test_the_rank_ordered_sum_is_the_row_sum_to_one_float_ulp(case):
    K, L, FC, W, H, F, Aspace, B = case
    ranks = sorted({n for c, n, _ in GRADIENT_CASES if c == case})
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B)
    _, G, R = oracle_tied_ranks(case, names, P, x, pi, v, ranks)
    seen = 0
    for n in ranks:
        for nm, g, r in zip(names, G, R[n]):
            if not is_batch_shaped(nm):
                continue
            assert r.dtype == np.float32 and r.shape == g.shape, nm
            ulp = np.spacing(np.abs(g).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(r.astype(np.float64) - g) <= ulp), (nm, n, float(np.abs(r - g).max()))
            seen += int(np.abs(g).max() > 1e-6)
    assert seen > 0
