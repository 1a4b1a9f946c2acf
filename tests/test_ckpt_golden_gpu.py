"""GPU: agz_trainer_save / agz_trainer_load against checkpoint files written BEFORE the codec (agogo_amd/csrc/ckpt.hpp) existed.

tests/golden/ckpt/ holds the twelve files — {plain, tied} x {no solver state, velocity, Adam} x {without, with running BatchNorm statistics} —
that the commit named in tests/golden/make_ckpt_goldens.py wrote for trainers whose every value was chosen on the host.  The same states,
rebuilt here, must save to exactly those bytes; each file must load into a fresh trainer and into trainers that hold the other kinds of
state (a velocity, Adam's moments, tracked statistics) with the documented result, read back through the getters; and a bad 01 / 02 file —
the forms that once were only partly checked before they were applied — must leave a differently initialised trainer untouched."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import agogo_amd as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ckpt_goldens", os.path.join(GOLDEN, "make_ckpt_goldens.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
E_INVALID = r"\(-1\)"


def golden(tied, state, bn):
    return os.path.join(GOLDEN, "ckpt", G.name(tied, state, bn))


def snapshot(t):
    """everything a checkpoint can touch, through the getters"""
    n = range(t.num_params())
    try:
        stats = [tuple(a.tobytes() for a in t.get_bn_stats(bi)) for bi in range(t.num_bn())]
    except A.AgzError:
        stats = None                                                     # N = 0: no estimates
    return {"params": [t.get_param(i).tobytes() for i in n], "solver": t.get_solver(), "adam": t.get_adam(),
            "velocity": [t.get_velocity(i).tobytes() for i in n], "moments": [tuple(a.tobytes() for a in t.get_moments(i)) for i in n],
            "tracking": t.get_bn_tracking(), "stats": stats}


def after_load(src, before, state, bn):
    """the documented state of a trainer that was `before` and loaded the file of a trainer that is `src`"""
    zeros = [bytes(len(p)) for p in src["params"]]
    want = {"params": src["params"], "velocity": zeros, "moments": [(z, z) for z in zeros]}
    if state == "none":                                                  # the options stay; the velocity, or the moments and t, are zeroed
        want["solver"], want["adam"] = before["solver"], dict(before["adam"], t=0)
    elif state == "velocity":                                            # the file's solver and velocity; Adam off
        want["solver"], want["velocity"], want["adam"] = src["solver"], src["velocity"], dict(before["adam"], on=False, t=0)
    else:                                                                # the file's solver, Adam settings, t and moments; a velocity is released
        want["solver"], want["adam"], want["moments"] = src["solver"], src["adam"], src["moments"]
    if bn:                                                               # the file's tracking setting and state
        want["tracking"], want["stats"] = src["tracking"], src["stats"]
    else:                                                                # N = 0, the setting stays
        want["tracking"], want["stats"] = dict(before["tracking"], weight=0.0), None
    return want


@pytest.mark.parametrize("tied,state,bn", G.STATES, ids=[G.name(*s)[:-4] for s in G.STATES])
def test_save_writes_the_golden_bytes_and_load_gives_the_documented_state(ctx, tmp_path, tied, state, bn):
    src = G.build_state(A, ctx, tied, state, bn)
    src.save(tmp_path / "saved.agz")
    want_bytes = open(golden(tied, state, bn), "rb").read()
    assert open(tmp_path / "saved.agz", "rb").read() == want_bytes
    s = snapshot(src)
    src.close()
    assert (s["stats"] is not None) == bn and s["adam"]["on"] == (state == "adam") and (s["solver"]["momentum"] != 0) == (state == "velocity")
    # into a fresh trainer, and into trainers that hold a velocity, Adam's moments, tracked statistics (N > 0)
    targets = [A.Trainer(ctx, *G.CASE, tied=tied), G.build_state(A, ctx, tied, "velocity", False, salt=3),
               G.build_state(A, ctx, tied, "adam", True, salt=5), G.build_state(A, ctx, tied, "none", True, salt=7)]
    for k, t in enumerate(targets):
        before = snapshot(t)
        assert before["params"] != s["params"]
        t.load(golden(tied, state, bn))
        assert snapshot(t) == after_load(s, before, state, bn), "target %d" % k
        t.save(tmp_path / "again.agz")                                   # ... and what it now holds is, where the file carries it all, the file
        if k == 0 or (state != "none" and bn):
            assert open(tmp_path / "again.agz", "rb").read() == want_bytes, "target %d" % k
        t.close()


def test_a_bad_01_or_02_file_changes_nothing(ctx, tmp_path):
    """cut, extended, or with a wrong count word in the LAST block: refused with every parameter, option and statistic as it was"""
    f01, f02 = open(golden(False, "none", False), "rb").read(), open(golden(False, "velocity", False), "rb").read()
    probe = A.Trainer(ctx, *G.CASE)
    n_last = probe.param_info(probe.num_params() - 1)[1]
    probe.close()
    at = len(f02) - 4 * n_last - 8                                       # the count word of the last tensor's velocity
    assert struct.unpack("<Q", f02[at:at + 8])[0] == n_last
    bad = [f01[:len(f01) - 4], f01[:len(f01) // 2], f01[:20], f01 + bytes(4), f02[:at] + struct.pack("<Q", n_last + 1) + f02[at + 8:],
           f02[:at] + struct.pack("<Q", n_last - 1) + f02[at + 8:]]
    targets = [G.build_state(A, ctx, False, "velocity", True, salt=3), G.build_state(A, ctx, False, "adam", True, salt=5)]
    for t in targets:
        before = snapshot(t)
        for k, blob in enumerate(bad):
            open(tmp_path / "bad.agz", "wb").write(blob)
            with pytest.raises(A.AgzError, match=E_INVALID):
                t.load(tmp_path / "bad.agz")
            assert snapshot(t) == before, "bad file %d" % k
        t.load(golden(False, "none", False))                             # (the trainer still loads the good file)
        assert snapshot(t)["params"] != before["params"]
        t.close()
