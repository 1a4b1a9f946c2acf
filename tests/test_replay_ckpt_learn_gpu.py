"""GPU: AZ.Learn stopped at an epoch boundary and resumed (agogo::AZ::SaveRun / LoadRun / Learn(..., first_epoch),
agogo_amd/host/agogo.hpp) on tic-tac-toe with a replay window, through the C++ host mirror over the C ABI (tests/cpp/az_learn_resume).

Run A is Learn(3, ...).  Run B is Learn(2, ...), SaveRun, and on a NEWLY constructed AZ LoadRun and Learn(1, ..., first_epoch = 2).  The
two print the same text: the epoch log with the cost as its bit pattern, wins, window and steps, the statistics, the network ids, the
digest of the final window and a digest of every parameter of A.  Before it resumes, run B hands its files to an AZ of another
configuration, and a ".run" file cut by one byte and a ".A" file that is not the one the ".run" was written beside to an AZ of the same:
all three are refused with nothing loaded.

Two processes can only be compared bit for bit where one run is bit-reproducible.  The trainer's weight gradients are summed with atomics
across batch tiles: at BatchSize 32 four uninterrupted runs of this binary gave three different parameter digests of A (the costs, read
before the last update, were the same bits), at BatchSize 8 — the batch of test_replay_gpu.py's trainers, whose bit-for-bit comparisons
rest on the same fact — and 16, six of six runs and every resumed one gave the same.  So BatchSize is 8 here.  The games are played once
by the synthetic inferencers of test_replay_learn_gpu.py and once by the networks themselves (the games of epoch 2 then depend on the A
that was loaded and on the B that was rebuilt)."""
import pytest

from test_replay_learn_gpu import INF_HASH, run

pytestmark = pytest.mark.gpu
KEPT = ("epoch", "stats", "ids", "window_digest", "a_params_digest")


@pytest.mark.parametrize("players", [INF_HASH, "0"], ids=["synthetic", "networks"])
@pytest.mark.parametrize("packed", [0, 1], ids=["fp32", "packed"])
def test_learn_resumed_at_an_epoch_boundary_is_the_uninterrupted_run(tmp_path, packed, players):
    inf = [players] * 4 + [8]                                            # the four inferencer kinds, BatchSize
    full = run("az_learn_resume", ["full", packed, tmp_path / "unused"] + inf)
    resumed = run("az_learn_resume", ["resume", packed, tmp_path / "run"] + inf)
    assert "AZ_LEARN_RESUME OK" in full.stdout and "AZ_LEARN_RESUME OK" in resumed.stdout, full.stdout + full.stderr + resumed.stdout + resumed.stderr
    a = [l for l in full.stdout.splitlines() if l.startswith(KEPT)]
    b = [l for l in resumed.stdout.splitlines() if l.startswith(KEPT)]
    assert len([l for l in a if l.startswith("epoch")]) == 3 and all(any(l.startswith(k) for l in a) for k in KEPT)
    assert a == b, "\n".join(["uninterrupted:"] + a + ["resumed:"] + b)
    refusals = [l for l in resumed.stdout.splitlines() if l.startswith("REFUSED")]
    assert len(refusals) == 3 and all("(named, nothing loaded)" in l for l in refusals), refusals
    assert "MCTSConf.Budget" in refusals[0] and "another configuration" in refusals[0] and "malformed" in refusals[1]
    assert "is not the trainer file" in refusals[2]
    for ext in (".A", ".window", ".run"):
        assert (tmp_path / ("run" + ext)).exists() and not (tmp_path / ("run" + ext + ".tmp")).exists()
    assert not (tmp_path / "unused.run").exists()
