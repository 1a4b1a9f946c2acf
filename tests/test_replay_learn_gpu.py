"""GPU: AZ.Learn with a replay window (agogo::Config::ReplayWindow, agogo_amd/host/agogo.hpp) on tic-tac-toe, through the C++ host mirror
over the C ABI (tests/cpp/az_learn_replay): the window lives across epochs, every epoch's examples join it, B trains on ReplaySteps
minibatches sampled from it.  With ReplayWindow = 0 the same binary runs the reference's loop, epoch log as az_learn_ttt prints it."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF_HASH = "3"


def run(name, args):
    exe = os.path.join(ROOT, "tests", "cpp", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", ROOT, "tests/cpp/" + name])
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    return out


def fields(line):
    w = line.split()
    return dict(zip(w[0::2], w[1::2]))


def test_az_learn_with_a_replay_window():
    iters, episodes, nniters, games, budget, batch, cap, steps = 3, 32, 2, 8, 20, 32, 300, 7
    out = run("az_learn_replay", [iters, episodes, nniters, games, budget, 0.52, 1337, 0, 0, 0, 0, batch, cap, steps, 1])
    assert "AZ_LEARN_REPLAY OK" in out.stdout, out.stdout + out.stderr
    log = [fields(l) for l in out.stdout.splitlines() if l.startswith("epoch")]
    assert len(log) == iters
    cumulative = 0
    for e in log:
        assert int(e["examples"]) >= episodes * 5                      # every tic-tac-toe game yields at least five examples
        cumulative += int(e["examples"])
        assert int(e["window"]) == min(cap, cumulative)                # the window's live rows: what was appended, up to its capacity
        assert int(e["steps"]) == steps                                # training ran ReplaySteps steps
        assert int(e["batches"]) == int(e["window"]) // batch
    assert cap < int(log[0]["examples"]) + int(log[1]["examples"])     # the window is smaller than two epochs' examples ...
    assert int(log[1]["window"]) == cap and int(log[2]["window"]) == cap   # ... so it wrapped, and stayed full


def test_replay_steps_default_and_window_off_is_the_reference_loop():
    # synthetic inferencers (the hooks of test_learn_parity_gpu.py): the games do not depend on fp32 rounding in a network evaluation
    base = [2, 32, 2, 8, 20, 0.52, 1337, INF_HASH, INF_HASH, INF_HASH, INF_HASH, 32]
    out = run("az_learn_replay", base + [200, 0, 0])                    # ReplaySteps = 0: (live / BatchSize) * nniters
    assert "AZ_LEARN_REPLAY OK" in out.stdout, out.stdout + out.stderr
    log = [fields(l) for l in out.stdout.splitlines() if l.startswith("epoch")]
    for e in log:
        assert int(e["steps"]) == (int(e["window"]) // 32) * 2 and int(e["steps"]) > 0
    off = run("az_learn_replay", base + [0, 0, 0])
    ttt = run("az_learn_ttt", base)
    assert "AZ_LEARN_REPLAY OK" in off.stdout and "AZ_LEARN OK" in ttt.stdout, off.stdout + off.stderr + ttt.stdout + ttt.stderr
    a = [l for l in off.stdout.splitlines() if l.startswith(("epoch", "stats"))]
    b = [l for l in ttt.stdout.splitlines() if l.startswith(("epoch", "stats"))]
    assert len(a) == len(b) >= 3
    for la, lb in zip(a, b):
        if la.startswith("stats"):
            assert la == lb
            continue
        fa, fb = fields(la), fields(lb)
        assert list(fa) == list(fb) and "window" not in fa
        # the cost of two runs of one training can differ in its last bits (sums accumulated with atomics): everything else is the same text
        ca, cb = float(fa.pop("cost")), float(fb.pop("cost"))
        assert fa == fb, (la, lb)
        assert abs(ca - cb) <= 1e-4 * max(1.0, abs(cb)), (la, lb)
