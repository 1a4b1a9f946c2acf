"""GPU: the trainer's running BatchNorm statistics (agz_trainer_set_bn_tracking), the forward-only pass that uses them (agz_trainer_eval),
their way into an inference net (agz_trainer_export -> AGZ_BN_RUNNING) and into checkpoints (AGZTRN03).

The declared rule (include/agz.h, DESIGN §2 `bn-running`), per BatchNorm op and channel, in double on the device:
    S_mean = lam * S_mean + mu_t;  S_var = lam * S_var + var_t;  N = lam * N + 1;   mean = (float)(S_mean / N), var = (float)(S_var / N)
with mu_t / var_t the batch mean / biased variance the forward normalises with.

Bars.  Statistics against a float64 restatement of the training forward: the project's training tolerance, 2e-5 of the tensor's scale
(mean: of max(max|mean|, max sqrt(var)); var: 4e-5 of max(var), a squared quantity carries twice the relative error).  The recurrence:
4 * 2^-24 * max_t |x_t[c]| per channel (the float rounding of each x_t read-back plus the final rounding).  eval against the forward it
was made from: the same bits where a step is reproducible, 2^-22 relative elsewhere (atomic summation order of the cost).  eval against
float64: 1e-4 * max(1, |cost|), the cost bar of test_train_gpu.  Played boards: POL_ATOL / POL_RTOL / VAL_ATOL of test_net_gpu."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import agogo_amd as A
import oracle_lib as O
from agogo_amd import capi
from test_net_gpu import POL_ATOL, POL_RTOL, VAL_ATOL
from test_solver_gpu import batch_data, make_dev, params, v1_file_size

pytestmark = pytest.mark.gpu

# K, L, FC, W, H, F, A, B: the smallest shapes that reach each finalize kernel (the heads' 2 + 1 channels are in all of them)
TWO_PASS = (32, 1, 16, 3, 3, 2, 10, 4)               # k_bn_sum + k_bn_fin
ODD_C = (3, 3, 8, 3, 3, 2, 10, 5)                    # C % 4 != 0
DETERMINISTIC = (32, 2, 24, 3, 3, 2, 10, 6)          # 54 rows: every reduction runs in one workgroup, a step reproduces to the bit
SINGLE_PASS = (32, 1, 16, 19, 19, 2, 362, 12)        # 4332 rows >= 4096: k_bn_stats + k_bn_fin2
MEASURED = (256, 1, 32, 19, 19, 18, 362, 12)         # AGZ_COMPUTE_WINO_H2 | FORCE: the measured step's k_bn_stats / k_bn_fin2 / k_bn_apply_v chain
SHAPES = {"TWO_PASS": TWO_PASS, "ODD_C": ODD_C, "DETERMINISTIC": DETERMINISTIC, "SINGLE_PASS": SINGLE_PASS, "MEASURED": MEASURED}
E_INVALID, E_STATE = r"\(-1\)", r"\(-4\)"


def mode_of(name):
    return "wino_h2" if name == "MEASURED" else None


def bn_stats(t):
    return [t.get_bn_stats(i) for i in range(t.num_bn())]


def torch_forward(P, case, x, pi, v, stats=None, eps=1e-5):
    """float64 restatement of the training forward (the conv_bn_relu chain of test_oracle_torch_xcheck): records mean / biased variance at
    every BatchNorm in op order; with `stats` (a list of (mean, var) per op) it normalises with those instead — the eval pass"""
    K, L, FC, W, H, F, Aspace, B = case
    P = [torch.tensor(np.asarray(p, np.float64)) for p in P]
    it = iter(range(len(P)))
    rec = []

    def conv_bn_relu(z, cin, cout, k):
        w = P[next(it)].reshape(cout, cin, k, k)
        g = P[next(it)].reshape(B, cout, H, W)
        b = P[next(it)].reshape(B, cout, H, W)
        y = Fn.conv2d(z, w, padding=k // 2)
        if stats is None:
            mean = y.mean(dim=(0, 2, 3), keepdim=True)
            var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        else:
            m, s = stats[len(rec)]
            mean = torch.tensor(np.asarray(m, np.float64)).reshape(1, cout, 1, 1)
            var = torch.tensor(np.asarray(s, np.float64)).reshape(1, cout, 1, 1)
        rec.append((mean.reshape(-1).numpy().copy(), var.reshape(-1).numpy().copy()))
        return torch.relu((y - mean) / torch.sqrt(var + eps) * g + b)

    z = conv_bn_relu(torch.tensor(x.astype(np.float64)), F, K, 3)
    for _ in range(L):
        a = conv_bn_relu(z, K, K, 3)
        b = conv_bn_relu(z, K, K, 3)
        z = torch.relu(a + b)
    p = conv_bn_relu(z, K, 2, 1).reshape(B, 2 * H * W)
    logits = p @ P[next(it)].reshape(2 * H * W, Aspace) + P[next(it)].reshape(B, Aspace)
    vv = conv_bn_relu(z, K, 1, 1).reshape(B, H * W)
    hid = torch.relu(vv @ P[next(it)].reshape(H * W, FC) + P[next(it)].reshape(B, FC))
    o = (hid @ P[next(it)].reshape(FC, 1) + P[next(it)].reshape(B, 1)).reshape(B)
    Pi, V = torch.tensor(pi.astype(np.float64)), torch.tensor(v.astype(np.float64))
    cost = -(Pi * logits + (1 - Pi) * (1 - logits)).mean() + ((o - V) ** 2).mean()
    return {"stats": rec, "logits": logits.numpy(), "o": o.numpy(), "cost": float(cost)}


def check_stats_against(got, want, tag):
    """test 3's bars, op by op; prints the worst fraction of the bar before asserting"""
    worst = [0.0, 0.0]
    fails = []
    for i, ((m, s), (m64, s64)) in enumerate(zip(got, want)):
        bar_m = 2e-5 * max(float(np.abs(m64).max()), float(np.sqrt(s64).max())) + 1e-9
        bar_v = 4e-5 * float(s64.max()) + 1e-12
        em, ev = float(np.abs(m - m64).max()), float(np.abs(s - s64).max())
        worst = [max(worst[0], em / bar_m), max(worst[1], ev / bar_v)]
        if em > bar_m or ev > bar_v:
            fails.append((i, em, bar_m, ev, bar_v))
    print("%s: worst mean error %.3f, worst variance error %.3f of the bar" % (tag, worst[0], worst[1]))
    assert not fails, (tag, fails)


# ---- 1. off is untouched ------------------------------------------------------------------------------------------------------------------
def test_tracking_changes_nothing_of_the_step_and_off_writes_the_01_file(ctx, tmp_path):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    ts = [make_dev(ctx, case, seed=21) for _ in range(2)]
    ts[1].set_bn_tracking(True, 0.9)
    for step in range(3):
        x, pi, v = batch_data(B, F, H, W, Aspace, seed=300 + step)
        costs = [t.batch(x, pi, v, lr=0.1) for t in ts]
        assert costs[0] == costs[1], (step, costs)
    for i, (p, q) in enumerate(zip(params(ts[0]), params(ts[1]))):
        assert p.tobytes() == q.tobytes(), ts[0].param_info(i)[0]
    assert ts[0].get_bn_tracking() == {"on": False, "momentum": np.float32(0.997), "weight": 0.0}
    path = tmp_path / "off.agz"
    ts[0].save(path)
    assert open(path, "rb").read(8) == b"AGZTRN01" and os.path.getsize(path) == v1_file_size(ts[0])
    assert ts[1].get_bn_tracking()["weight"] > 2.0


# ---- 2. the first step is exact, whatever the momentum --------------------------------------------------------------------------------------
def test_first_step_gives_the_same_estimates_for_every_momentum(ctx):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=310)
    dt = make_dev(ctx, case, seed=21)
    ref = None
    for lam in (0.0, 0.5, 0.997):
        dt.reset_bn_stats()
        dt.set_bn_tracking(True, lam)
        dt.forward_backward(x, pi, v)
        st = dt.get_bn_tracking()
        assert st["weight"] == 1.0 and st["on"] and st["momentum"] == np.float32(lam)
        got = bn_stats(dt)
        assert len(got) == dt.num_bn() == 2 * L + 3
        assert [m.size for m, _ in got] == [K] * (2 * L + 1) + [2, 1]
        if ref is None:
            ref = got
        for i in range(len(got)):
            assert got[i][0].tobytes() == ref[i][0].tobytes() and got[i][1].tobytes() == ref[i][1].tobytes(), (lam, i)


# ---- 3. the statistics against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_statistics_against_the_float64_forward(ctx, name):
    case = SHAPES[name]
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5, mode=mode_of(name))
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=320)
    dt.set_bn_tracking(True, 0.0)
    cost = dt.forward_backward(x, pi, v)
    ref = torch_forward(params(dt), case, x, pi, v)
    print("%s: cost %.7f (float64 %.7f)" % (name, cost, ref["cost"]))
    check_stats_against(bn_stats(dt), ref["stats"], name)


# ---- 4. the recurrence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TWO_PASS", "SINGLE_PASS"])
def test_three_forwards_follow_the_declared_recurrence(ctx, name):
    case = SHAPES[name]
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5)
    batches = [batch_data(B, F, H, W, Aspace, seed=330 + k) for k in range(3)]
    dt.set_bn_tracking(True, 0.0)
    xs = []
    for b in batches:                 # (lr = 0: forward_backward takes no step, the learnables are the same for every batch)
        dt.reset_bn_stats()
        dt.forward_backward(*b)
        xs.append(bn_stats(dt))
    dt.reset_bn_stats()
    dt.set_bn_tracking(True, 0.9)
    for b in batches:
        dt.forward_backward(*b)
    lam = np.float64(np.float32(0.9))
    n = lam * lam + lam + 1
    assert abs(dt.get_bn_tracking()["weight"] - n) <= 1e-12
    got = bn_stats(dt)
    worst = 0.0
    for i in range(dt.num_bn()):
        for k in range(2):
            x1, x2, x3 = (xs[t][i][k].astype(np.float64) for t in range(3))
            want = (lam * lam * x1 + lam * x2 + x3) / n
            bar = 4 * 2.0 ** -24 * np.maximum(np.maximum(np.abs(x1), np.abs(x2)), np.abs(x3))
            err = np.abs(got[i][k].astype(np.float64) - want)
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()) if bar.max() > 0 else 0.0)
            assert (err <= bar).all(), (i, k, float(err.max()), float(bar.min()))
    print("%s: recurrence, worst %.3f of the bar" % (name, worst))


# ---- 5. eval equals the forward it was made from ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_returns_the_cost_of_the_forward_it_was_made_from(ctx, name):
    case = SHAPES[name]
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5, mode=mode_of(name))
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=340)
    with pytest.raises(capi.AgzError, match=E_STATE):
        dt.eval(x, pi, v)
    dt.set_bn_tracking(True, 0.997)
    cost = dt.forward_backward(x, pi, v)
    before = (params(dt), [dt.get_grad(i) for i in range(dt.num_params())], bn_stats(dt), dt.get_bn_tracking())
    ev = dt.eval(x, pi, v)
    print("%s: forward %.9g eval %.9g" % (name, cost, ev))
    if name == "DETERMINISTIC":
        assert np.float32(ev).tobytes() == np.float32(cost).tobytes(), (cost, ev)
    else:
        assert abs(ev - cost) <= 2.0 ** -22 * abs(cost), (cost, ev)
    after = (params(dt), [dt.get_grad(i) for i in range(dt.num_params())], bn_stats(dt), dt.get_bn_tracking())
    for k in range(2):
        for i, (p, q) in enumerate(zip(before[k], after[k])):
            assert p.tobytes() == q.tobytes(), (k, dt.param_info(i)[0])
    for (m0, s0), (m1, s1) in zip(before[2], after[2]):
        assert m0.tobytes() == m1.tobytes() and s0.tobytes() == s1.tobytes()
    assert before[3] == after[3] and after[3]["weight"] == 1.0
    dt.set_bn_tracking(False, 0.997)          # off keeps the state: eval still works
    assert abs(dt.eval(x, pi, v) - ev) <= (0.0 if name == "DETERMINISTIC" else 2.0 ** -22 * abs(ev))


# ---- 6. eval against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TWO_PASS", "SINGLE_PASS"])
def test_eval_of_a_held_out_batch_against_float64(ctx, name):
    case = SHAPES[name]
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5)
    dt.set_bn_tracking(True, 0.9)
    for k in range(3):
        dt.batch(*batch_data(B, F, H, W, Aspace, seed=350 + k), lr=0.05)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=353)
    ev = dt.eval(x, pi, v)
    ref = torch_forward(params(dt), case, x, pi, v, stats=bn_stats(dt))
    print("%s: eval %.7f float64 %.7f" % (name, ev, ref["cost"]))
    assert abs(ev - ref["cost"]) <= 1e-4 * max(1.0, abs(ref["cost"])), (ev, ref["cost"])
    assert abs(dt.get_bn_tracking()["weight"] - 2.71) < 1e-6


# ---- 7. plays as trained ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TWO_PASS", "SINGLE_PASS", "MEASURED"])
def test_exported_net_plays_the_boards_as_the_training_forward_saw_them(ctx, name):
    case = SHAPES[name]
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5, mode=mode_of(name))
    row0 = []
    for i in range(dt.num_params()):          # every batch-shaped tensor: row 0 in all B rows (inference knows row 0 alone)
        nm, n = dt.param_info(i)
        p = dt.get_param(i)
        if nm.endswith(("_gamma", "_beta", "_b")):
            p = np.tile(p[:n // B], B)
            dt.set_param(i, p)
            row0.append(p[:n // B])
        else:
            row0.append(p)
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=360)
    ref = torch_forward(params(dt), case, x, pi, v)
    e = np.exp(ref["logits"] - ref["logits"].max(axis=1, keepdims=True))
    pol64, val64 = e / e.sum(axis=1, keepdims=True), np.tanh(ref["o"])
    net = A.Net(ctx, K, L, FC, W, H, F, Aspace, BatchSize=B, bn_mode=capi.BN_RUNNING)

    def meets(pol, val):
        return np.allclose(pol, pol64, atol=POL_ATOL, rtol=POL_RTOL) and np.allclose(val, val64, atol=VAL_ATOL)

    dt.forward_backward(x, pi, v)             # not tracked: the export carries no statistics, the net keeps mean 0 / var 1
    dt.export(net)
    assert not meets(*net.infer(x)), "an export without statistics already plays as trained"
    dt.set_bn_tracking(True, 0.997)
    dt.forward_backward(x, pi, v)
    dt.export(net)
    pol, val = net.infer(x)
    print("%s: policy error %.3g, value error %.3g" % (name, np.abs(pol - pol64).max(), np.abs(val - val64).max()))
    np.testing.assert_allclose(pol, pol64, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(val, val64, atol=VAL_ATOL)
    onet = O.Net(K, L, FC, W, H, F, Aspace, BatchSize=B, bn_mode=1)
    for i, p in enumerate(row0):
        onet.set_param(i, p)
    for i, (m, s) in enumerate(bn_stats(dt)):
        onet.set_bn_stats(i, m, s)
    pol_o, val_o = onet.infer(x)
    np.testing.assert_allclose(pol, pol_o, atol=POL_ATOL, rtol=POL_RTOL)
    np.testing.assert_allclose(val, val_o, atol=VAL_ATOL)


# ---- 8. checkpoint ----------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_statistics_and_a_cut_file_changes_nothing(ctx, tmp_path):
    case = DETERMINISTIC
    K, L, FC, W, H, F, Aspace, B = case
    batches = [batch_data(B, F, H, W, Aspace, seed=370 + k) for k in range(3)]

    def state(t):
        return (params(t), [t.get_velocity(i) for i in range(t.num_params())], bn_stats(t), t.get_bn_tracking())

    def same(a, b):
        return (all(p.tobytes() == q.tobytes() for k in range(2) for p, q in zip(a[k], b[k])) and
                all(m0.tobytes() == m1.tobytes() and s0.tobytes() == s1.tobytes() for (m0, s0), (m1, s1) in zip(a[2], b[2])) and a[3] == b[3])

    dt = make_dev(ctx, case, seed=21)
    dt.set_solver(0.9, 0.0, 0.0)
    dt.set_bn_tracking(True, 0.9)
    for b in batches[:2]:
        dt.batch(*b, lr=0.1)
    path = tmp_path / "bn.agz"
    dt.save(path)
    blob = open(path, "rb").read()
    assert blob[:8] == b"AGZTRN03" and blob[8:12] == (2).to_bytes(4, "little")
    bn_block = 12 + sum(16 + 16 * c for c in [K] * (2 * L + 1) + [2, 1])
    assert len(blob) == 12 + 2 * (v1_file_size(dt) - 8) - 48 + 16 + bn_block     # magic + form, the 02 body, the BatchNorm block
    dt.batch(*batches[2], lr=0.1)
    want = state(dt)

    other = make_dev(ctx, case, seed=99)
    other.load(path)
    assert other.get_bn_tracking() == {"on": True, "momentum": np.float32(0.9), "weight": np.float64(np.float32(0.9)) + 1}
    other.batch(*batches[2], lr=0.1)
    assert same(state(other), want)

    # a file cut inside the magic, the inner body, the BatchNorm header, an op's S_mean, and by its last byte: rejected, nothing changed
    untouched = state(other)
    for cut in (5, 100, len(blob) - bn_block + 6, len(blob) - bn_block + 12 + 16 + 4, len(blob) - 1):
        bad = tmp_path / ("cut%d.agz" % cut)
        open(bad, "wb").write(blob[:cut])
        with pytest.raises(capi.AgzError, match=E_INVALID):
            other.load(bad)
        assert same(state(other), untouched), cut

    # an 01 file into a tracking trainer: no statistics, the setting kept
    plain = make_dev(ctx, case, seed=21)
    plain.save(tmp_path / "v1.agz")
    assert open(tmp_path / "v1.agz", "rb").read(8) == b"AGZTRN01"
    other.load(tmp_path / "v1.agz")
    assert other.get_bn_tracking() == {"on": True, "momentum": np.float32(0.9), "weight": 0.0}
    with pytest.raises(capi.AgzError, match=E_STATE):
        other.get_bn_stats(0)


# ---- 9. validation ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_and_change_nothing(ctx):
    case = TWO_PASS
    K, L, FC, W, H, F, Aspace, B = case
    dt = make_dev(ctx, case, seed=5)
    dt.set_bn_tracking(True, 0.5)
    for on, lam in ((2, 0.5), (-1, 0.5), (1, -0.1), (1, 1.0), (1, float("nan")), (1, float("inf"))):
        with pytest.raises(capi.AgzError, match=E_INVALID):
            dt.set_bn_tracking(on, lam)
        assert dt.get_bn_tracking() == {"on": True, "momentum": 0.5, "weight": 0.0}
    with pytest.raises(capi.AgzError, match=E_STATE):
        dt.get_bn_stats(0)
    ones = np.ones(K, np.float32)
    with pytest.raises(capi.AgzError, match=E_INVALID):
        dt.set_bn_stats(0, ones[:K - 1], ones[:K - 1], 1.0)
    with pytest.raises(capi.AgzError, match=E_INVALID):
        dt.set_bn_stats(dt.num_bn() - 1, ones[:2], ones[:2], 1.0)      # the value head has one channel
    for w in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.AgzError, match=E_INVALID):
            dt.set_bn_stats(0, ones, ones, w)
    with pytest.raises(capi.AgzError, match=E_INVALID):
        dt.set_bn_stats(dt.num_bn(), ones, ones, 1.0)
    dt.set_bn_stats(0, 2 * ones, 3 * ones, 4.0)                          # S = weight * value, N = weight
    m, s = dt.get_bn_stats(0)
    assert (m == 2).all() and (s == 3).all() and dt.get_bn_tracking()["weight"] == 4.0
    x, pi, v = batch_data(B, F, H, W, Aspace, seed=380)
    with pytest.raises(capi.AgzError, match=E_STATE):                    # the other ops still have N = 0
        dt.eval(x, pi, v)
    dt.reset_bn_stats()
    assert dt.get_bn_tracking() == {"on": True, "momentum": 0.5, "weight": 0.0}
