"""GPU: the tied-affine trainer (agz_trainer_create_tied; include/agz.h, DESIGN §2 `tied-affine`): BatchNorm gamma / beta [C,H,W] and FC
biases [units] stored once and shared by every batch row.

Reference: the oracle with the tied tensor in every row of its batch-shaped tensors, its per-row gradients summed over the row axis in
float64 (test_tied_cpu.oracle_tied, checked there against a float64 torch model with tied tensors).  Bars: the project's gradient bar
(2e-5 of the tensor's largest expected element, test_train_gpu) and cost bar (1e-5); trajectories: test_sgd_steps_and_export's; played
boards: test_net_gpu's.  Where the declared definition promises the same bits (the forward of an untied trainer holding the tiled rows,
B = 1, two runs on one batch, fused against two-pass where every reduction of a step runs in one workgroup) the comparison is on bytes.

Shapes: test_adam_gpu.CASES and (32,1,16,3,3,2,10,33): k_bn_bwd1_tied splits the batch rows into TB_RS = 4 interleaved slices, 33 rows
are more than, and no multiple of, 4 (and more than the 8-row tiles of the FC kernels)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi
from test_adam_cpu import adam_step
from test_adam_gpu import B1, B2, CASES, DETERMINISTIC, FUSED_CASE, HEADLINE, _splitmix, grads, moments, params, rel_diff
from test_net_gpu import POL_ATOL, POL_RTOL, VAL_ATOL
from test_solver_gpu import solver_step
from test_tied_cpu import batch_data, draw_tied, is_batch_shaped, oracle_tied

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
ODD_ROWS = (32, 1, 16, 3, 3, 2, 10, 33)
B_ONE = (20, 1, 8, 4, 4, 2, 17, 1)
E_INVALID, E_STATE = r"\(-1\)", r"\(-4\)"
MODES = {"f32": None, "bf16x3": capi.COMPUTE_BF16X3 | capi.COMPUTE_FORCE, "wino_h2": capi.COMPUTE_WINO_H2 | capi.COMPUTE_FORCE}


def make_tied(ctx, case, names, P, mode="f32"):
    t = A.Trainer(ctx, *case, tied=True)
    if MODES[mode] is not None:
        t.set_compute_mode(MODES[mode])
    for i, p in enumerate(P):
        t.set_param(i, p)
    return t


def make_untied(ctx, case, names, P, mode="f32"):
    """a plain trainer holding the tied tensor in every row"""
    B = case[-1]
    t = A.Trainer(ctx, *case)
    if MODES[mode] is not None:
        t.set_compute_mode(MODES[mode])
    for i, (nm, p) in enumerate(zip(names, P)):
        t.set_param(i, np.tile(p, B) if is_batch_shaped(nm) else p)
    return t


def row_sum(names, G, B):
    return [g.astype(np.float64).reshape(B, -1).sum(axis=0) if is_batch_shaped(nm) else g.astype(np.float64) for nm, g in zip(names, G)]


# ---- 1. shapes --------------------------------------------------------------------------------------------------------------------------------
def test_a_tied_trainer_has_the_inference_nets_shapes(ctx):
    case = CASES[1]
    K, L, FC, W, H, F, Aspace, B = case
    t, u = A.Trainer(ctx, *case, tied=True), A.Trainer(ctx, *case)
    net = A.Net(ctx, K, L, FC, W, H, F, Aspace, BatchSize=B)
    assert t.is_tied() and not u.is_tied()
    assert t.num_params() == net.num_params() == u.num_params()
    for i in range(t.num_params()):
        assert t.param_info(i) == net.param_info(i), i
        assert u.param_info(i)[0] == t.param_info(i)[0]
        assert u.param_info(i)[1] == t.param_info(i)[1] * (B if is_batch_shaped(t.param_info(i)[0]) else 1)
    # init_random: row 0 of what the plain trainer draws
    t.init_random(11)
    u.init_random(11)
    for i in range(t.num_params()):
        a, b = t.get_param(i), u.get_param(i)
        assert a.tobytes() == b[:a.size].tobytes(), t.param_info(i)[0]
    for h in (t, u, net):
        h.close()


# ---- 2. gradient against the oracle ------------------------------------------------------------------------------------------------------
def check_gradient(ctx, case, mode, data_seed=None):
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=K + B if data_seed is None else data_seed)
    co, GO = oracle_tied(case, names, P, x, pi, v)
    dt = make_tied(ctx, case, names, P, mode)
    cd = dt.forward_backward(x, pi, v)
    GD = grads(dt)
    dt.close()
    print("case %s mode %s: cost %.9g oracle %.9g" % (case, mode, cd, co))
    assert abs(cd - co) <= 1e-5 * max(1.0, abs(co)), (cd, co)
    missed, worst = [], 0.0
    for i, (nm, go, gd) in enumerate(zip(names, GO, GD)):
        assert gd.shape == go.shape, (nm, gd.shape, go.shape)
        scale = float(np.abs(go).max())
        err = float(np.abs(gd - go).max())
        worst = max(worst, err / (2e-5 * scale + 1e-7))
        if err > 2e-5 * scale + 1e-7:
            missed.append((i, nm, err, scale))
    print("    worst tensor %.3f of the gradient bar" % worst)
    if missed:
        # the rule of the issue for a summed tensor that misses the bar: the plain trainer on the same draw, its row gradients summed the same
        # way, sets the scale (err_tied <= 2 * err_untied, the margin DESIGN §9 uses between arithmetic modes)
        ut = make_untied(ctx, case, names, P, mode)
        ut.forward_backward(x, pi, v)
        GU = row_sum(names, grads(ut), B)
        ut.close()
        for i, nm, err, scale in missed:
            eu = float(np.abs(GU[i] - GO[i]).max())
            print("    %s: err_tied %.3e err_untied %.3e scale %.3e" % (nm, err, eu, scale))
            assert is_batch_shaped(nm) and err <= 2 * eu, (nm, err, eu, scale)
    assert any(np.abs(g).max() > 1e-6 for nm, g in zip(names, GO) if is_batch_shaped(nm))


@pytest.mark.parametrize("case", CASES + [ODD_ROWS])
def test_gradient_is_the_row_sum_of_the_oracles(ctx, case):
    check_gradient(ctx, case, "f32")


def test_gradient_bf16x3(ctx):
    check_gradient(ctx, CASES[3], "bf16x3")


def test_gradient_at_the_headline_width_wino_h2(ctx):
    """the shape of test_forward_backward_headline_width_19x19 (test_train_gpu) on the first of that test's data draws, seed 77"""
    check_gradient(ctx, HEADLINE, "wino_h2", data_seed=77)


# ---- 3. forward equals the untied forward; 4. B = 1; 5. reproducible -----------------------------------------------------------------------
def test_forward_is_the_untied_forward_to_the_bit(ctx):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=31)
    dt, ut = make_tied(ctx, case, names, P), make_untied(ctx, case, names, P)
    ct, cu = dt.forward_backward(x, pi, v), ut.forward_backward(x, pi, v)
    assert np.float32(ct).tobytes() == np.float32(cu).tobytes(), (ct, cu)
    dt.close()
    ut.close()


def test_with_one_row_every_gradient_is_the_untied_trainers_to_the_bit(ctx):
    case = B_ONE
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=32)
    dt, ut = make_tied(ctx, case, names, P), make_untied(ctx, case, names, P)
    assert dt.forward_backward(x, pi, v) == ut.forward_backward(x, pi, v)
    for nm, a, b in zip(names, grads(dt), grads(ut)):
        assert a.tobytes() == b.tobytes(), nm
    assert any(g.any() for g in grads(dt))
    dt.close()
    ut.close()


def test_two_runs_on_one_batch_give_the_same_bits(ctx):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=33)
    dt = make_tied(ctx, case, names, P)
    dt.forward_backward(x, pi, v)
    g1 = [g.tobytes() for g in grads(dt)]
    dt.forward_backward(x, pi, v)
    for nm, a, b in zip(names, g1, grads(dt)):
        assert a == b.tobytes(), nm
    dt.close()


# ---- 6. fused = two-pass ---------------------------------------------------------------------------------------------------------------------
def solver_state(t):
    return [a.tobytes() for a in params(t)], [t.get_velocity(i).tobytes() for i in range(t.num_params())], [(m.tobytes(), u.tobytes()) for m, u in moments(t)]


def run_pair(ctx, case, kind, eps, steps=3):
    """(fused, two-pass) tied trainers after `steps` steps of the solver `kind`"""
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case, seed=21)
    pair = [make_tied(ctx, case, names, P) for _ in range(2)]
    lr = 0.1
    for t in pair:
        if kind == "l2clip":
            t.set_solver(0, 1e-4, 10 * eps)
        elif kind == "momentum":
            t.set_solver(0.9, 1e-4, 0)
        elif kind == "adam":
            t.set_adam(B1, B2, eps)
            t.set_solver(0, 1e-4, 0)
    if kind == "adam":
        lr = 0.1 * eps                       # (test_adam_gpu: the Lipschitz constant lr / eps* of Adam's map = the vanilla pair's learn rate)
    for step in range(steps):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        pair[0].batch(x, pi, v, lr=lr)
        pair[1].forward_backward(x, pi, v)
        pair[1].apply(lr)
    return pair


def tied_eps_star(ctx, case):
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case, seed=21)
    t = make_tied(ctx, case, names, P)
    t.forward_backward(*batch_data(B, F, H, W, Aspace, seed=300))
    e = float(np.median(np.concatenate([np.abs(g) for g in grads(t)])))
    t.close()
    assert e > 0
    return e


def test_fused_step_equals_the_two_pass_step_for_every_solver(ctx):
    """as test_adam_gpu.check_fused_equals_two_pass: every solver's pair within 3 * max(e0, 2e-6) per tensor, e0 the vanilla pair's own
    difference in this run (the vanilla pair itself: test_fused_gamma_beta_step_equals_the_two_pass_step's 2e-6 after that test's TWO steps —
    the spread comes from the float atomics of the head convolution's weight gradient and grows with every step)"""
    case = FUSED_CASE
    eps = tied_eps_star(ctx, case)
    van2 = run_pair(ctx, case, "vanilla", eps, steps=2)
    e2 = [rel_diff(a, b) for a, b in zip(params(van2[0]), params(van2[1]))]
    print("vanilla pair after two steps: worst %.2e" % max(e2))
    assert max(e2) <= 2e-6, e2
    for t in van2:
        t.close()
    van = run_pair(ctx, case, "vanilla", eps)
    pf, pt = params(van[0]), params(van[1])
    e0 = [rel_diff(a, b) for a, b in zip(pf, pt)]
    print("vanilla pair after three steps: worst %.2e" % max(e0))
    for kind in ("l2clip", "momentum", "adam"):
        f, t = run_pair(ctx, case, kind, eps)
        fails, worst = [], 0.0
        for i, (a, b) in enumerate(zip(params(f), params(t))):
            e = rel_diff(a, b)
            worst = max(worst, e / (3 * max(e0[i], 2e-6)))
            if not e <= 3 * max(e0[i], 2e-6):
                fails.append((f.param_info(i)[0], e, e0[i]))
        if kind == "momentum":
            assert any(f.get_velocity(i).any() for i in range(f.num_params()))
            for i in range(f.num_params()):
                assert rel_diff(f.get_velocity(i), t.get_velocity(i)) <= 3 * max(e0[i], 2e-6), f.param_info(i)[0]
        if kind == "adam":
            assert f.get_adam()["t"] == 3 == t.get_adam()["t"] and any(m.any() for m, _ in moments(f))
        print("%s pair: worst %.2f of the bar" % (kind, worst))
        assert not fails, (kind, fails)
        f.close()
        t.close()
    for t in van:
        t.close()


@pytest.mark.parametrize("kind", ["vanilla", "l2clip", "momentum", "adam"])
def test_fused_step_is_the_two_pass_step_to_the_bit_where_a_step_is_one_workgroup(ctx, kind):
    """both paths step the tied gamma / beta through the one out-of-line tied_step (train.hip), everything else through k_solver_sweep"""
    f, t = run_pair(ctx, DETERMINISTIC, kind, tied_eps_star(ctx, DETERMINISTIC))
    sf, st = solver_state(f), solver_state(t)
    for i in range(f.num_params()):
        assert sf[0][i] == st[0][i] and sf[1][i] == st[1][i] and sf[2][i] == st[2][i], (kind, f.param_info(i)[0])
    f.close()
    t.close()


# ---- 7. trajectories against numpy over the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_trajectory_matches_numpy_over_the_oracle(ctx, kind):
    """test_adam_trajectory_matches_numpy_over_the_oracle / test_momentum_trajectory_...: CASES[0], seed 9, wscale 1.0, L2 1e-4, three steps of
    batch(lr); the oracle re-tiled each step supplies the row-summed gradients, float32 numpy carries the state.  Bars: cost 2e-5,
    parameters 1e-4 * max|w| + 1e-7 per tensor."""
    case = CASES[0]
    K, L, FC, W, H, F, Aspace, B = case
    l2 = 1e-4
    names, P = draw_tied(case, seed=9, wscale=1.0)
    dt = make_tied(ctx, case, names, P)
    w = [p.copy() for p in P]
    m = [np.zeros_like(a) for a in w]
    u = [np.zeros_like(a) for a in w]
    if kind == "adam":
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=100)
        _, G0 = oracle_tied(case, names, w, x, pi, v)
        eps = float(np.median(np.concatenate([np.abs(g) for g in G0])))
        lr = 1e-3
        dt.set_adam(B1, B2, eps)
        dt.set_solver(0, l2, 0)
    else:
        lr = 0.02
        dt.set_solver(0.9, l2, 0)
    for step in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=100 + step)
        co, G = oracle_tied(case, names, w, x, pi, v)
        for i in range(len(w)):
            g = G[i].astype(np.float32)
            if kind == "adam":
                w[i], m[i], u[i], _, _ = adam_step(w[i], m[i], u[i], g, lr, 1.0, l2, 0, B1, B2, eps, step + 1)
            else:
                w[i], m[i], _ = solver_step(w[i], m[i], g, lr, 1.0, 0.9, l2, 0)
        cd = dt.batch(x, pi, v, lr=lr)
        assert abs(cd - co) <= 2e-5 * max(1.0, abs(co)), (step, cd, co)
    worst = 0.0
    for i in range(len(w)):
        scale, err = float(np.abs(w[i]).max()), float(np.abs(dt.get_param(i) - w[i]).max())
        worst = max(worst, err / (1e-4 * scale + 1e-7))
        assert err <= 1e-4 * scale + 1e-7, (names[i], err, scale)
    print("%s trajectory against numpy over the oracle: worst parameter error %.3f of the bar" % (kind, worst))
    dt.close()


# ---- 8. plays as trained ---------------------------------------------------------------------------------------------------------------------
def test_the_exported_net_is_the_trained_state_and_plays_every_board_as_trained(ctx):
    from test_bn_tracking_gpu import bn_stats, torch_forward
    case = CASES[1]
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    dt = make_tied(ctx, case, names, P)
    dt.set_bn_tracking(True, 0.997)
    dt.batch(*batch_data(B, F, H, W, Aspace, seed=359), lr=0.01)       # (a trained state: every tied tensor has moved)
    dt.reset_bn_stats()
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=360)
    cost = dt.forward_backward(x, pi, v)                                # ONE tracked forward
    net = A.Net(ctx, K, L, FC, W, H, F, Aspace, BatchSize=B, bn_mode=capi.BN_RUNNING)
    dt.export(net)
    for i in range(dt.num_params()):
        assert net.get_param(i).tobytes() == dt.get_param(i).tobytes(), names[i]
        assert dt.get_param(i).tobytes() != P[i].tobytes(), names[i]
    # that forward itself, restated in float64 (training-mode BatchNorm, the tied tensor in every row): its policy and value for EVERY board
    # of the batch, no equal-rows precondition, and its cost (test_bn_tracking_gpu's reference and bars)
    trained = [dt.get_param(i) for i in range(dt.num_params())]
    ref = torch_forward([np.tile(p, B) if is_batch_shaped(nm) else p for nm, p in zip(names, trained)], case, x, pi, v)
    e = np.exp(ref["logits"] - ref["logits"].max(axis=1, keepdims=True))
    pol64, val64 = e / e.sum(axis=1, keepdims=True), np.tanh(ref["o"])
    assert abs(cost - ref["cost"]) <= 1e-4 * max(1.0, abs(ref["cost"])), (cost, ref["cost"])
    pol, val = net.infer(x)
    print("policy error %.3g, value error %.3g against the float64 training forward" % (np.abs(pol - pol64).max(), np.abs(val - val64).max()))
    assert np.abs(pol64 - pol64[0]).max() > 1e-4
    np.testing.assert_allclose(pol, pol64, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(val, val64, atol=VAL_ATOL)
    # ... and the oracle's inference net under the same statistics
    onet = O.Net(K, L, FC, W, H, F, Aspace, BatchSize=B, bn_mode=1)
    for i in range(dt.num_params()):
        onet.set_param(i, dt.get_param(i))
    for i, (mm, ss) in enumerate(bn_stats(dt)):
        onet.set_bn_stats(i, mm, ss)
    pol_o, val_o = onet.infer(x)
    np.testing.assert_allclose(pol, pol_o, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(val, val_o, atol=VAL_ATOL)
    ev = dt.eval(x, pi, v)
    assert abs(ev - cost) <= 2.0 ** -22 * abs(cost), (ev, cost)
    dt.close()
    net.close()


# ---- 9. checkpoints ---------------------------------------------------------------------------------------------------------------------------
def full_state(t):
    from test_bn_tracking_gpu import bn_stats
    return (t.get_adam(), t.get_solver(), solver_state(t), t.get_bn_tracking(), [(a.tobytes(), b.tobytes()) for a, b in bn_stats(t)])


def test_checkpoint_round_trip_and_the_tied_flag(ctx, tmp_path):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    t1 = make_tied(ctx, case, names, P)
    t1.set_adam(0.8, 0.99, 1e-6)
    t1.set_solver(0, 1e-4, 0.5)
    t1.set_bn_tracking(True, 0.9)
    for s in (1, 2):
        t1.batch(*batch_data(B, F, H, W, Aspace, seed=s), lr=0.01)
    path = tmp_path / "tied.agz"
    t1.save(path)
    blob = open(path, "rb").read()
    assert blob[:8] == b"AGZTRN05" and struct.unpack("<III", blob[8:20]) == (3, 1, 3)     # inner form 03 (its own inner form 3: Adam), flags = tied
    t2 = A.Trainer(ctx, *case, tied=True)
    t2.load(path)
    assert full_state(t2) == full_state(t1) and t2.get_adam()["t"] == 2
    for t in (t1, t2):
        t.batch(*batch_data(B, F, H, W, Aspace, seed=3), lr=0.01)
    assert full_state(t2) == full_state(t1) and t2.get_adam()["t"] == 3
    # tied file -> plain trainer, plain file -> tied trainer: refused, nothing changed
    plain = A.Trainer(ctx, *case)
    plain.init_random(4)
    before = solver_state(plain)
    with pytest.raises(A.AgzError, match=E_INVALID):
        plain.load(path)
    assert solver_state(plain) == before
    plain.save(tmp_path / "plain.agz")
    pb = open(tmp_path / "plain.agz", "rb").read()
    assert pb[:8] == b"AGZTRN01" and len(pb) == 8 + 40 + 8 + sum(8 + 4 * plain.param_info(i)[1] for i in range(plain.num_params()))
    again = A.Trainer(ctx, *case)
    again.load(tmp_path / "plain.agz")                                  # the plain file is what it always was: it re-loads to the same bits
    assert solver_state(again)[0] == before[0]
    before2 = full_state(t2)
    with pytest.raises(A.AgzError, match=E_INVALID):
        t2.load(tmp_path / "plain.agz")
    assert full_state(t2) == before2
    # truncated and inconsistent 05 files
    bad = tmp_path / "bad.agz"
    for b in [blob[:c] for c in (8, 12, 16, 20, 60, len(blob) // 2, len(blob) - 8, len(blob) - 1)] + [blob + b"\0", blob[:12] + struct.pack("<I", 3) + blob[16:],
                                                                                                 blob[:12] + struct.pack("<I", 0) + blob[16:],
                                                                                                 blob[:8] + struct.pack("<I", 5) + blob[12:]]:
        open(bad, "wb").write(b)
        with pytest.raises(A.AgzError, match=E_INVALID):
            t2.load(bad)
    assert full_state(t2) == before2
    # a tied trainer without solver state or statistics: inner form 1, every truncation rejected as well
    t3 = make_tied(ctx, case, names, P)
    t3.save(tmp_path / "tied1.agz")
    b1 = open(tmp_path / "tied1.agz", "rb").read()
    assert b1[:8] == b"AGZTRN05" and struct.unpack("<II", b1[8:16]) == (1, 1) and len(b1) == 16 + 40 + 8 + sum(8 + 4 * p.size for p in P)
    open(bad, "wb").write(b1[:-4])
    with pytest.raises(A.AgzError, match=E_INVALID):
        t2.load(bad)
    assert full_state(t2) == before2
    for t in (t1, t2, t3, plain, again):
        t.close()


def test_with_one_row_the_flag_alone_tells_the_files_apart(ctx, tmp_path):
    case = B_ONE
    names, P = draw_tied(case)
    tied, plain = make_tied(ctx, case, names, P), make_untied(ctx, case, names, [2 * p for p in P])
    assert [tied.param_info(i) for i in range(tied.num_params())] == [plain.param_info(i) for i in range(plain.num_params())]
    tied.save(tmp_path / "t.agz")
    plain.save(tmp_path / "p.agz")
    st, sp = solver_state(tied), solver_state(plain)
    with pytest.raises(A.AgzError, match=E_INVALID):
        plain.load(tmp_path / "t.agz")
    with pytest.raises(A.AgzError, match=E_INVALID):
        tied.load(tmp_path / "p.agz")
    assert solver_state(tied) == st and solver_state(plain) == sp
    tied.close()
    plain.close()


# ---- 10. refusals; 11. train_dev ---------------------------------------------------------------------------------------------------------------
def test_the_sliced_allreduce_refuses_a_tied_handle(ctx):
    case = CASES[0]
    K, L, FC, W, H, F, Aspace, B = case
    names, P = draw_tied(case)
    dt = make_tied(ctx, case, names, P)
    comm = A.Comm.init_all([ctx])[0]
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=1)
    before = solver_state(dt)
    with pytest.raises(A.AgzError, match=E_STATE):
        comm.forward_backward_allreduce(dt, x, pi, v)
    assert solver_state(dt) == before
    comm.close()
    dt.close()


def test_train_dev_on_a_tied_trainer_is_a_loop_of_batch(ctx):
    case = (32, 1, 16, 3, 3, 2, 10, 8)        # test_train_dev_with_adam_is_a_loop_of_batch's
    K, L, FC, W, H, F, Aspace, B = case
    batches, iterations, seed = 3, 2, 11
    x, pi, v = batch_data(B * batches, F, H, W, Aspace, seed=1)
    ex = A.Examples(ctx, F, H, W, Aspace)
    ex.append_host(x, pi, v)
    assert ex.prepare(B, 0, seed=77) == batches
    xd, pd, vd, _, _ = ex.tensors_dev()
    xs, ps, vs = [np.array(a) for a in ex.tensors()]
    xs = xs.reshape(B * batches, F, H, W)
    names, P = draw_tied(case, seed=3)
    t1, t2 = make_tied(ctx, case, names, P), make_tied(ctx, case, names, P)
    t0 = make_tied(ctx, case, names, P)
    t0.forward_backward(xs[:B], ps[:B], vs[:B])
    eps = float(np.median(np.concatenate([np.abs(g) for g in grads(t0)])))
    t0.close()
    for t in (t1, t2):
        t.set_adam(B1, B2, eps)
        t.set_solver(0, 1e-4, 0)
    c1 = t1.train_dev(xd, pd, vd, batches, iterations, seed=seed)
    perm = list(range(B * batches))
    rng = _splitmix(seed)
    for it in range(iterations):
        for b in range(batches):
            rows = perm[b * B:(b + 1) * B]
            c2 = t2.batch(xs[rows], ps[rows], vs[rows], lr=0.1)
        for i in range(len(perm)):
            j = next(rng) % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
    assert abs(c1 - c2) <= 1e-5 * max(1.0, abs(c2)), (c1, c2)
    assert t1.get_adam()["t"] == batches * iterations == t2.get_adam()["t"]
    assert any(m.any() for m, _ in moments(t1))
    ex.close()
    t1.close()
    t2.close()


# ---- 12. agz_trainer_allreduce over two ranks ------------------------------------------------------------------------------------------------
WORKER = r"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import agogo_amd as A
from test_tied_cpu import batch_data, draw_tied
rank, n, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
ctx = A.Ctx(0)
idf = out + ".uid"
if rank == 0:
    uid = A.Comm.unique_id()
    with open(idf + ".tmp", "wb") as f:
        f.write(uid)
    os.replace(idf + ".tmp", idf)
else:
    t0 = time.time()
    while not os.path.exists(idf):
        assert time.time() - t0 < 60, "rank 0 never published the unique id"
        time.sleep(0.01)
    uid = open(idf, "rb").read()
comm = A.Comm.init_rank(ctx, n, rank, uid)
case = (32, 1, 16, 3, 3, 2, 10, 4)
names, P = draw_tied(case)
tr = A.Trainer(ctx, *case, tied=True)
for i, p in enumerate(P):
    tr.set_param(i, p)
x, pi, v = batch_data(4, 2, 3, 3, 10, seed=100 + rank)
tr.forward_backward(x, pi, v)
local = [tr.get_grad(i).copy() for i in range(tr.num_params())]
comm.allreduce_trainer(tr)
ctx.sync()
summed = [tr.get_grad(i).copy() for i in range(tr.num_params())]
tr.apply(0.1, 1.0 / n)
ctx.sync()
after = [tr.get_param(i).copy() for i in range(tr.num_params())]
np.savez(out + ".r%d.npz" % rank, nparams=tr.num_params(), **{"local%d" % i: g for i, g in enumerate(local)},
         **{"sum%d" % i: g for i, g in enumerate(summed)}, **{"after%d" % i: g for i, g in enumerate(after)})
comm.close()
"""


def test_allreduce_over_two_ranks_steps_both_on_the_summed_gradient(tmp_path):
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is built by `make` (__graft_entry__.build)"
    n = 2
    out = str(tmp_path / "x")
    env = dict(os.environ, AGZ_RCCL_LIB=FAKE)
    procs = [subprocess.Popen([sys.executable, "-c", WORKER, str(r), str(n), out], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(n)]
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-3000:])
    R = [np.load(out + ".r%d.npz" % r) for r in range(n)]
    names, P = draw_tied((32, 1, 16, 3, 3, 2, 10, 4))
    for i in range(int(R[0]["nparams"])):
        s = (R[0]["local%d" % i] + R[1]["local%d" % i]).astype(np.float32)
        assert s.size == P[i].size                                       # the tied shapes went through the collective
        for r in range(n):
            np.testing.assert_array_equal(R[r]["sum%d" % i], s)
            np.testing.assert_array_equal(R[r]["after%d" % i], R[0]["after%d" % i])
        np.testing.assert_allclose(R[0]["after%d" % i], P[i] - np.float32(0.1 / n) * s, rtol=2e-6, atol=1e-7)
    assert not np.array_equal(R[0]["local1"], R[1]["local1"])
