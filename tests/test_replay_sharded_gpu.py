"""GPU: the sharded replay route (agz_replay_sample_slice*, agz_replay_digest, agz_train_replay_sharded; include/agz.h, DESIGN §2
`replay-sharded`, §7).

The slice sampler is compared byte for byte with Replay.sample of the same window, the device digest with agz_replay_digest_host of
Replay.get (the definition itself is restated in Python integers in test_replay_sharded_cpu.py).  The collective trainer runs on ranks that
are processes on GPU 0 through tests/fake_rccl (AGZ_RCCL_LIB), in the worker pattern of test_tied_sharded_gpu.py: at most two ranks, every
rank under its own time limit, a non-zero or timed-out rank fails the test.  Its reference is sharded train_dev on the same communicator
over the global minibatches Replay.sample gives, under the rule of test_replay_gpu.py: the reference runs twice, and if it is bit-reproducible
the replay run must equal it bit for bit — parameters, solver state and cost — else within that test's 1e-4 of a tensor's largest magnitude."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
from test_replay_packed_gpu import PALETTES, pal_floats, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
INVALID, STATE, UNSUPPORTED = -1, -4, -6
ROWS = 8
SLICES = [(0, ROWS), (0, 3), (3, ROWS - 3), (ROWS - 1, 1)]
SHAPES = [  # H, W, F, A1, cap, palette of the packed window
    pytest.param(3, 3, 2, 10, 9, "twoplane", id="3x3"),
    pytest.param(5, 5, 3, 26, 11, "wq", id="5x5"),
    pytest.param(19, 19, 18, 362, 40, "wq", id="19x19"),
]
CONF = (32, 1, 16, 3, 3, 2, 10, 8)        # K, blocks, FC, W, H, F, A, global B
TRAIN_CAP, TRAIN_ROWS, STEPS, SEED = 12, 20, 3, 4242


def make_rows(rng, n, F, H, W, A1, pal):
    planes = rng.choice(np.array(PALETTES[pal], np.uint32), size=(n, F * H * W)).astype(np.uint32).view(np.float32)
    return planes, rng.normal(size=(n, A1)).astype(np.float32), rng.normal(size=n).astype(np.float32)


def windows(ctx, H, W, F, A1, cap, pal):
    return A.Replay(ctx, F, H, W, A1, cap), A.Replay(ctx, F, H, W, A1, cap, palette=pal_floats(pal))


@pytest.mark.parametrize("H,W,F,A1,cap,pal", SHAPES)
def test_slices_are_the_rows_of_the_whole_minibatch(ctx, H, W, F, A1, cap, pal):
    rng = np.random.default_rng(H + A1)
    plain, packed = windows(ctx, H, W, F, A1, cap, pal)
    buf = A.Examples(ctx, F, H, W, A1)                                   # device buffers for sample_slice_dev, and their read-back
    buf.append_host(*[np.zeros_like(a) for a in make_rows(rng, ROWS, F, H, W, A1, pal)])
    out = A.Examples(ctx, F, H, W, A1)
    bx, bp, bv = buf.raw_dev()
    for state, n in (("partly filled", cap - 3), ("wrapped", 8)):
        rows = make_rows(rng, n, F, H, W, A1, pal)
        for rp in (plain, packed):
            rp.append_host(*rows)
        assert len(plain) == (cap - 3 if state == "partly filled" else cap) and plain.total() == (cap - 3 if state == "partly filled" else cap + 5)
        for rp, kind in ((plain, "unpacked"), (packed, "packed")):
            for step in (0, 5):
                for symmetric in (False, True):
                    msg = "%s %s step %d symmetric %d" % (state, kind, step, symmetric)
                    whole = rp.sample(ROWS, 77, step, symmetric)
                    assert all(same(a, b) for a, b in zip(whole, plain.sample(ROWS, 77, step, symmetric))), msg
                    for row0, cnt in SLICES:
                        got = rp.sample_slice(ROWS, row0, cnt, 77, step, symmetric)
                        for a, w in zip(got, whole):
                            assert same(a, w[row0:row0 + cnt]), (msg, row0, cnt)
                        rp.sample_slice_dev(ROWS, row0, cnt, 77, step, symmetric, bx, bp, bv)
                        out.clear()
                        out.append_dev(bx, bp, bv, cnt)
                        for a, w in zip(out.get(), whole):
                            assert same(a.reshape(w[row0:row0 + cnt].shape), w[row0:row0 + cnt]), (msg, row0, cnt, "sample_slice_dev")
                    parts = [rp.sample_slice(ROWS, r0, c, 77, step, symmetric) for r0, c in ((0, 3), (3, ROWS - 3))]
                    for i, w in enumerate(whole):                       # concatenated slices are the whole batch
                        assert same(np.concatenate([parts[0][i], parts[1][i]]), w), msg
    for h in (plain, packed, buf, out):
        h.close()


def test_slice_refusals(ctx):
    L = capi.lib()
    F, S, A1 = 2, 3, 10
    rp = A.Replay(ctx, F, S, S, A1, 6)
    x, p, v = np.zeros((ROWS, F, S, S), np.float32), np.zeros((ROWS, A1), np.float32), np.zeros(ROWS, np.float32)
    buf = A.Examples(ctx, F, S, S, A1)
    buf.append_host(x.reshape(ROWS, -1), p, v)
    bx, bp, bv = (C.c_void_p(a) for a in buf.raw_dev())
    host = lambda rows, row0, cnt, sym=0: L.agz_replay_sample_slice(rp.h, rows, row0, cnt, 1, 0, sym, capi._pf(x), capi._pf(p), capi._pf(v))
    dev = lambda rows, row0, cnt, sym=0: L.agz_replay_sample_slice_dev(rp.h, rows, row0, cnt, 1, 0, sym, bx, bp, bv)
    for call in (host, dev):
        assert call(ROWS, 0, ROWS) == STATE                              # an empty window
        assert b"empty" in L.agz_last_error()
    rp.append_host(*make_rows(np.random.default_rng(1), 4, F, S, S, A1, "twoplane"))
    for call in (host, dev):
        assert call(ROWS, 0, ROWS) == 0
        assert call(ROWS, -1, 2) == INVALID                              # row0 < 0
        assert call(ROWS, 0, 0) == INVALID and call(ROWS, 2, -1) == INVALID      # cnt < 1
        assert call(ROWS, 6, 3) == INVALID and call(ROWS, ROWS, 1) == INVALID    # row0 + cnt > rows
        assert call(ROWS, 1, 2 ** 31 - 1) == INVALID                     # ... without wrapping
        assert call(0, 0, 1) == INVALID                                  # rows < 1
        assert b"row0" in L.agz_last_error()
    with pytest.raises(capi.AgzError):
        rp.sample_slice(ROWS, 6, 3, 1)
    # the symmetric preconditions are the whole sampler's, with its messages
    ns = A.Replay(ctx, F, 2, 3, 7, 4)
    ns.append_host(*make_rows(np.random.default_rng(2), 2, F, 2, 3, 7, "twoplane"))
    assert L.agz_replay_sample_slice(ns.h, ROWS, 0, 2, 1, 0, 1, capi._pf(x), capi._pf(p), capi._pf(v)) == INVALID
    assert b"square boards" in L.agz_last_error()
    assert L.agz_replay_sample_slice(ns.h, ROWS, 0, 2, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == 0
    for h in (rp, ns, buf):
        h.close()


def host_digest(rp):
    return capi.replay_digest_host(*rp.get(), rp.F, rp.H * rp.W, rp.A1)


@pytest.mark.parametrize("H,W,F,A1,cap,pal", SHAPES)
def test_the_device_digest_is_the_host_digest_of_the_logical_rows(ctx, H, W, F, A1, cap, pal):
    rng = np.random.default_rng(3 * H + A1)
    plain, packed = windows(ctx, H, W, F, A1, cap, pal)
    assert plain.digest() == packed.digest() == 0                        # empty: digest = live = 0
    seen = set()
    for n in (1, cap - 4, 8):                                            # one row; partly filled; wrapped
        rows = make_rows(rng, n, F, H, W, A1, pal)
        for rp in (plain, packed):
            rp.append_host(*rows)
        d = plain.digest()
        assert d == host_digest(plain)
        assert packed.digest() == d == host_digest(packed)               # packed and unpacked, fed the same rows
        assert plain.digest() == d                                       # the same call: the same value
        assert d not in seen                                             # ... and another one after every append
        seen.add(d)
    assert plain.total() == cap + 5
    # the same logical content by another route: one append of the live rows into a fresh window, whose ring has not wrapped
    live = plain.get()
    for other in windows(ctx, H, W, F, A1, cap + 3, pal):
        other.append_host(*live)
        assert other.total() == cap and other.digest() == d
        other.append_host(*[a[:1] for a in live])                        # one more append: another digest
        assert other.digest() != d
        other.close()
    # a window of the same capacity whose ring sits at another physical offset
    for shifted in windows(ctx, H, W, F, A1, cap, pal):
        shifted.append_host(*make_rows(rng, 2, F, H, W, A1, pal))
        shifted.append_host(*live)
        assert shifted.total() == cap + 2 and shifted.digest() == d
        shifted.close()
    # the order of the rows counts, and so does the sign of a zero
    p, q, v = live
    assert capi.replay_digest_host(p[::-1], q[::-1], v[::-1], F, H * W, A1) != d
    z = q.copy()
    z[0, 0] = 0.0
    dz = capi.replay_digest_host(p, z, v, F, H * W, A1)
    z[0, 0] = -0.0
    assert capi.replay_digest_host(p, z, v, F, H * W, A1) != dz
    for h in (plain, packed):
        h.close()


def test_a_plain_handle_is_refused(ctx):
    """agz_train_replay_sharded is the sharded handles' call: a plain trainer is AGZ_E_STATE, pointed to agz_train_replay, nothing trained"""
    L = capi.lib()
    K, blocks, FC, W, H, F, Aspace, B = CONF
    rp = A.Replay(ctx, F, H, W, Aspace, 6)
    rp.append_host(*make_rows(np.random.default_rng(1), 4, F, H, W, Aspace, "twoplane"))
    for tied in (False, True):
        t = A.Trainer(ctx, K, blocks, FC, W, H, F, Aspace, B, tied=tied)
        t.init_random(9)
        before = [t.get_param(i) for i in range(t.num_params())]
        cost = C.c_float(0)
        assert L.agz_train_replay_sharded(t.h, rp.h, 1, 1, 0, 1, C.byref(cost)) == STATE
        assert b"agz_train_replay" in L.agz_last_error() and b"not a sharded" in L.agz_last_error()
        with pytest.raises(capi.AgzError):
            t.train_replay_sharded(rp, 1)
        for i, b in enumerate(before):
            assert t.get_param(i).tobytes() == b.tobytes()
        t.close()
    rp.close()


WORKER = r"""
import ctypes as C
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import agogo_amd as A
from agogo_amd import capi
rank, n, spec = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
jobs = json.load(open(spec))
ctx = A.Ctx(0)
idf = spec + ".uid"
if rank == 0:
    with open(idf + ".tmp", "wb") as f:
        f.write(A.Comm.unique_id())
    os.replace(idf + ".tmp", idf)
else:
    t0 = time.time()
    while not os.path.exists(idf):
        assert time.time() - t0 < 60, "rank 0 never published the unique id"
        time.sleep(0.01)
comm = A.Comm.init_rank(ctx, n, rank, open(idf, "rb").read())

def err(fn):
    try:
        fn()
    except A.AgzError as e:
        return str(e)
    return ""

def make(job, tied, adam):
    t = A.Trainer.sharded(ctx, comm, *job["conf"], tied=tied)
    t.init_random(9)
    if adam:
        t.set_adam()
    return t

def state(t, res, tag):
    for i in range(t.num_params()):
        res["%sp%d" % (tag, i)] = t.get_param(i)
        res["%sv%d" % (tag, i)] = t.get_velocity(i)
        m1, m2 = t.get_moments(i)
        res["%sm%d" % (tag, i)], res["%su%d" % (tag, i)] = m1, m2
    res["%st" % tag] = np.int64(t.get_adam()["t"])

def window(job, rows, palette=None):
    K, L, FC, W, H, F, Aspace, Bg = job["conf"]
    rp = A.Replay(ctx, F, H, W, Aspace, job["cap"], palette=palette)
    rp.append_host(*rows)
    return rp

for ji, job in enumerate(jobs):
    K, L, FC, W, H, F, Aspace, Bg = job["conf"]
    inp = np.load(job["inp"])
    rows = (inp["x"], inp["pi"], inp["v"])
    steps, seed = job.get("steps", 3), job.get("seed", 1)
    res = {}
    kind = job["kind"]
    if kind == "train":        # every rank builds the same window; replay-sharded against sharded train_dev over the sampled global batches
        rp, packed = window(job, rows), window(job, rows, inp["palette"])
        res["counts"] = np.array([len(rp), rp.total(), len(packed), packed.total()])
        mb = [rp.sample(Bg, seed, s, True) for s in range(steps)]
        ex = A.Examples(ctx, F, H, W, Aspace)
        ex.append_host(np.concatenate([m[0] for m in mb]).reshape(steps * Bg, -1), np.concatenate([m[1] for m in mb]), np.concatenate([m[2] for m in mb]))
        xd, pd, vd = ex.raw_dev()
        for tied in (0, 1):
            for adam in (0, 1):
                tag = "%s_%s_" % ("tied" if tied else "plain", "adam" if adam else "sgd")
                ref1, ref2, run, runp = (make(job, tied, adam) for _ in range(4))
                res[tag + "shard"] = np.array(run.shard())
                state(run, res, tag + "init_")
                res[tag + "ref1_cost"] = np.float32(ref1.train_dev(xd, pd, vd, steps, 1, seed=5))
                res[tag + "ref2_cost"] = np.float32(ref2.train_dev(xd, pd, vd, steps, 1, seed=5))
                res[tag + "run_cost"] = np.float32(run.train_replay_sharded(rp, steps, seed, True, True))
                res[tag + "runp_cost"] = np.float32(runp.train_replay_sharded(packed, steps, seed, True, True))
                for t, name in ((ref1, "ref1_"), (ref2, "ref2_"), (run, "run_"), (runp, "runp_")):
                    state(t, res, tag + name)
                before = [run.get_param(i).tobytes() for i in range(run.num_params())]
                res[tag + "zero_cost"] = np.float32(run.train_replay_sharded(rp, 0, seed, True, True))       # no step: nothing happens
                res[tag + "zero_same"] = np.array(before == [run.get_param(i).tobytes() for i in range(run.num_params())])
                for t in (ref1, ref2, run, runp):
                    t.close()
        # unchanged: agz_train_replay still refuses a sharded handle
        t = make(job, 1, 0)
        cost = C.c_float(0)
        res["plain_call_rc"] = np.int64(capi.lib().agz_train_replay(t.h, rp.h, 1, 1, 0, C.byref(cost)))
        res["plain_call_msg"] = np.array(capi.lib().agz_last_error().decode())
        t.close()
        for h in (ex, rp, packed):
            h.close()
    elif kind == "identity":   # n = 1: the tied sharded handle from a window against the tied trainer's agz_train_replay
        rp = window(job, rows)
        for adam in (0, 1):
            tag = "adam_" if adam else "sgd_"
            s = make(job, 1, adam)
            p = A.Trainer(ctx, K, L, FC, W, H, F, Aspace, Bg, tied=True)
            p.init_random(9)
            if adam:
                p.set_adam()
            res[tag + "s_cost"] = np.float32(s.train_replay_sharded(rp, steps, seed, True, True))
            res[tag + "p_cost"] = np.float32(p.train_replay(rp, steps, seed, True))
            state(s, res, tag + "s_")
            state(p, res, tag + "p_")
            s.close()
            p.close()
        rp.close()
    elif kind == "disagree":   # rank 1's replica differs: by one row (count), then by one policy value (same counts)
        x, pi, v = rows
        r0 = rank * (Bg // n)
        fb = (np.ascontiguousarray(inp["bx"][r0:r0 + Bg // n]), np.ascontiguousarray(inp["bpi"][r0:r0 + Bg // n]), np.ascontiguousarray(inp["bv"][r0:r0 + Bg // n]))
        short = window(job, rows if rank == 0 else tuple(a[:-1] for a in rows))
        res["short_counts"] = np.array([len(short), short.total()])
        pi2 = pi.copy()
        if rank == 1:
            pi2[-2, 3] = np.nextafter(pi2[-2, 3], np.float32(9))
        other = window(job, (x, pi2, v))
        res["other_counts"] = np.array([len(other), other.total()])
        res["other_digest"] = np.uint64(other.digest())
        for tied in (0, 1):
            tag = "tied_" if tied else "plain_"
            t = make(job, tied, 0)
            before = [t.get_param(i).tobytes() for i in range(t.num_params())]
            for verify in (0, 1):                                   # the counts are compared with or without the digest
                res[tag + "short_msg%d" % verify] = np.array(err(lambda: t.train_replay_sharded(short, steps, seed, True, bool(verify))))
            res[tag + "other_msg"] = np.array(err(lambda: t.train_replay_sharded(other, steps, seed, True, True)))
            res[tag + "untouched"] = np.array(before == [t.get_param(i).tobytes() for i in range(t.num_params())])
            res[tag + "next_cost"] = np.float32(t.forward_backward(*fb))       # the next collective call on the communicator works
            res[tag + "noverify_cost"] = np.float32(t.train_replay_sharded(other, steps, seed, True, False))
            res[tag + "trained"] = np.array(before != [t.get_param(i).tobytes() for i in range(t.num_params())])
            t.close()
        short.close()
        other.close()
    np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


def run_ranks(n, jobs, tmp_path, tag, timeout=120):
    """n rank processes on GPU 0 run `jobs` (collectively, in order), each under its own time limit; returns [job][rank] -> npz"""
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is built by `make` (__graft_entry__.build)"
    for j, job in enumerate(jobs):
        job["out"] = str(tmp_path / ("%s_j%d_r%%d.npz" % (tag, j)))
    spec = str(tmp_path / ("%s.json" % tag))
    with open(spec, "w") as f:
        json.dump(jobs, f)
    env = dict(os.environ, AGZ_RCCL_LIB=FAKE)
    procs = [subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, "-c", WORKER, str(r), str(n), spec], cwd=ROOT, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n)]
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=timeout + 30)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed (%d):\n%s" % (r, pr.returncode, logs[r][-3000:])
    return [[np.load(job["out"] % r) for r in range(n)] for job in jobs]


def train_inputs(tmp_path):
    """TRAIN_ROWS rows for a cap-TRAIN_CAP window of the two-rank shape (planes from the twoplane palette, so that they pack), and one
    global batch for a forward_backward"""
    K, blocks, FC, W, H, F, Aspace, Bg = CONF
    rng = np.random.default_rng(3)
    x, _, _ = make_rows(rng, TRAIN_ROWS, F, H, W, Aspace, "twoplane")
    pi = np.zeros((TRAIN_ROWS, Aspace), np.float32)
    pi[np.arange(TRAIN_ROWS), rng.integers(0, Aspace, TRAIN_ROWS)] = 1
    v = rng.choice(np.array([-1, 0, 1], np.float32), TRAIN_ROWS).astype(np.float32)
    path = str(tmp_path / "rows.npz")
    np.savez(path, x=x, pi=pi, v=v, palette=pal_floats("twoplane"), bx=x[:Bg].reshape(Bg, F, H, W), bpi=pi[:Bg], bv=v[:Bg])
    return path


STATE_KEYS = ("p", "v", "m", "u")


def states_equal(R, a, b, n_params, exact, label):
    """handle a's parameters, solver state and cost against handle b's: bytes if exact, else test_replay_gpu.py's 1e-4 bar"""
    ca, cb = float(R[a + "cost"]), float(R[b + "cost"])
    if exact:
        assert ca == cb, (label, ca, cb)
    else:
        assert abs(ca - cb) <= 1e-4 * max(1.0, abs(cb)), (label, ca, cb)
    assert int(R[a + "t"]) == int(R[b + "t"]), label
    for i in range(n_params):
        for k in STATE_KEYS:
            x, y = R["%s%s%d" % (a, k, i)], R["%s%s%d" % (b, k, i)]
            if exact:
                assert x.tobytes() == y.tobytes(), (label, k, i)
            else:
                assert np.abs(x - y).max() <= 1e-4 * max(np.abs(y).max(), 1e-3), (label, k, i)


def n_params_of(R, tag):
    return len([k for k in R.files if k.startswith(tag + "run_p")])


def test_two_ranks_train_on_the_global_minibatches(tmp_path):
    """train_replay_sharded(steps = 3, verify = 1) on two ranks (B = 4 each) — plain and tied handles, SGD and Adam, an unpacked and a packed
    window — against sharded train_dev(batches = 3, iterations = 1) over Replay.sample(8, seed, step) of steps 0..2 stacked in step order"""
    job = {"kind": "train", "conf": CONF, "cap": TRAIN_CAP, "steps": STEPS, "seed": SEED, "inp": train_inputs(tmp_path)}
    R = run_ranks(2, [job], tmp_path, "train")[0]
    for r in range(2):
        assert R[r]["counts"].tolist() == [TRAIN_CAP, TRAIN_ROWS, TRAIN_CAP, TRAIN_ROWS]      # the ring has wrapped
        assert int(R[r]["plain_call_rc"]) == UNSUPPORTED and "sharded" in str(R[r]["plain_call_msg"])
    for tag in ("plain_sgd_", "plain_adam_", "tied_sgd_", "tied_adam_"):
        n_params = n_params_of(R[0], tag)
        assert n_params > 0
        for r in range(2):
            Rr = R[r]
            assert Rr[tag + "shard"].tolist() == [4 * r, 4, 2]
            reproducible = all(Rq[tag + "ref1_cost"].tobytes() == Rq[tag + "ref2_cost"].tobytes() and
                               all(Rq["%sref1_%s%d" % (tag, k, i)].tobytes() == Rq["%sref2_%s%d" % (tag, k, i)].tobytes()
                                   for i in range(n_params) for k in STATE_KEYS) for Rq in R)
            print("%s rank %d: sharded train_dev run-to-run bit-reproducible: %s; cost replay %.9g, packed %.9g, train_dev %.9g"
                  % (tag, r, reproducible, Rr[tag + "run_cost"], Rr[tag + "runp_cost"], Rr[tag + "ref1_cost"]))
            assert any(Rr["%srun_p%d" % (tag, i)].tobytes() != Rr["%sinit_p%d" % (tag, i)].tobytes() for i in range(n_params))   # it trained
            assert int(Rr[tag + "run_t"]) == (STEPS if "adam" in tag else 0)
            states_equal(Rr, tag + "run_", tag + "ref1_", n_params, reproducible, tag + "replay against train_dev, rank %d" % r)
            states_equal(Rr, tag + "runp_", tag + "run_", n_params, reproducible, tag + "packed against unpacked, rank %d" % r)
            assert float(Rr[tag + "zero_cost"]) == 0.0 and bool(Rr[tag + "zero_same"])
        for name in ("run_cost", "runp_cost"):                           # the cost is the global one, the same bits on both ranks
            assert R[0][tag + name].tobytes() == R[1][tag + name].tobytes(), (tag, name)


def test_one_rank_tied_is_train_replay_on_the_tied_trainer(tmp_path):
    """§7's n = 1 promise: train_replay_sharded on a 1-rank communicator equals agz_train_replay on agz_trainer_create_tied, bit for bit"""
    job = {"kind": "identity", "conf": CONF, "cap": TRAIN_CAP, "steps": STEPS, "seed": SEED, "inp": train_inputs(tmp_path)}
    R = run_ranks(1, [job], tmp_path, "identity")[0][0]
    for tag in ("sgd_", "adam_"):
        n_params = len([k for k in R.files if k.startswith(tag + "s_p")])
        assert n_params > 0
        states_equal(R, tag + "s_", tag + "p_", n_params, True, tag + "one rank against the tied trainer")


def test_disagreeing_replicas_are_refused_on_every_rank(tmp_path):
    """rank 1 holds one row fewer: AGZ_E_STATE on both ranks with or without verify, nothing changed, the communicator still works.  Equal
    counts and one differing policy value: verify = 1 refuses on both ranks, verify = 0 trains — the documented meaning of the flag."""
    job = {"kind": "disagree", "conf": CONF, "cap": TRAIN_CAP, "steps": STEPS, "seed": SEED, "inp": train_inputs(tmp_path)}
    R = run_ranks(2, [job], tmp_path, "disagree")[0]
    assert R[0]["short_counts"].tolist() == [TRAIN_CAP, TRAIN_ROWS] and R[1]["short_counts"].tolist() == [TRAIN_CAP, TRAIN_ROWS - 1]
    assert R[0]["other_counts"].tolist() == R[1]["other_counts"].tolist() == [TRAIN_CAP, TRAIN_ROWS]
    assert int(R[0]["other_digest"]) != int(R[1]["other_digest"])
    for tag in ("plain_", "tied_"):
        for r in range(2):
            Rr = R[r]
            for verify in (0, 1):
                msg = str(Rr[tag + "short_msg%d" % verify])
                assert "(%d)" % STATE in msg and "rank 1" in msg and "total" in msg, (tag, r, verify, msg)
            msg = str(Rr[tag + "other_msg"])
            assert "(%d)" % STATE in msg and "rank 1" in msg and "digest" in msg, (tag, r, msg)
            assert bool(Rr[tag + "untouched"]), (tag, r)
            assert np.isfinite(float(Rr[tag + "next_cost"]))
            assert np.isfinite(float(Rr[tag + "noverify_cost"])) and bool(Rr[tag + "trained"]), (tag, r)
        assert R[0][tag + "next_cost"].tobytes() == R[1][tag + "next_cost"].tobytes()
