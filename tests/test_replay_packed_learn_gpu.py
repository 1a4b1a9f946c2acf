"""GPU: AZ.Learn with a packed replay window (agogo::Config::ReplayPacked, agogo_amd/host/agogo.hpp) on tic-tac-toe, through the C++ host
mirror over the C ABI (tests/cpp/az_learn_replay_packed): the same run with the window's planes kept as 2-bit codes under
agz_encoder_palette(AGZ_ENC_TWOPLANE) and as fp32 rows.  The sampler gives the trainer the same bits either way, so the two epoch logs are
the same text; only the window is smaller."""
import pytest

from test_replay_learn_gpu import INF_HASH, fields, run

pytestmark = pytest.mark.gpu


def test_a_packed_window_learns_what_an_unpacked_one_learns():
    # the arguments of test_replay_learn_gpu.py::test_replay_steps_default_and_window_off_is_the_reference_loop: synthetic inferencers, so
    # the games do not depend on fp32 rounding in a network evaluation; window 200, ReplaySteps = 0, symmetric off
    base = [2, 32, 2, 8, 20, 0.52, 1337, INF_HASH, INF_HASH, INF_HASH, INF_HASH, 32, 200, 0, 0]
    on = run("az_learn_replay_packed", base + [1])
    off = run("az_learn_replay_packed", base + [0])
    assert "AZ_LEARN_REPLAY_PACKED OK" in on.stdout and "AZ_LEARN_REPLAY_PACKED OK" in off.stdout, on.stdout + on.stderr + off.stdout + off.stderr
    a = [l for l in on.stdout.splitlines() if l.startswith(("epoch", "stats"))]
    b = [l for l in off.stdout.splitlines() if l.startswith(("epoch", "stats"))]
    assert len(a) == len(b) >= 3
    epochs = 0
    for la, lb in zip(a, b):
        if la.startswith("stats"):
            assert la == lb
            continue
        fa, fb = fields(la), fields(lb)
        assert list(fa) == list(fb) and "window_bytes" in fa
        # the cost of two runs of one training can differ in its last bits (sums accumulated with atomics): everything else is the same text
        ca, cb = float(fa.pop("cost")), float(fb.pop("cost"))
        wa, wb = int(fa.pop("window_bytes")), int(fb.pop("window_bytes"))
        assert fa == fb, (la, lb)
        assert abs(ca - cb) <= 1e-4 * max(1.0, abs(cb)), (la, lb)
        # 3x3, 2 planes, policy 10: one word a plane against nine floats
        assert wa == 200 * (2 * 1 * 4 + 10 * 4 + 4) and wb == 200 * (2 * 9 + 10 + 1) * 4 and wa < wb, (la, lb)
        assert int(fa["steps"]) == (int(fa["window"]) // 32) * 2 and int(fa["steps"]) > 0
        epochs += 1
    assert epochs == 2
