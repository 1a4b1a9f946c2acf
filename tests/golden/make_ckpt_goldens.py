"""Writes the trainer-checkpoint fixtures tests/golden/ckpt/*.agz (tests/test_ckpt_golden_gpu.py compares against them).

The committed fixtures were written ONCE, on a gfx950 device, by the build of commit 08c06e7 ("Trainer: tied gamma/beta and FC biases
shared by every batch row") — the last commit whose train.hip held the checkpoint code itself, before it moved into csrc/ckpt.hpp.  They
pin the file format: do not regenerate them with the code under test.  Usage (from the repository root, after `make`):

    python tests/golden/make_ckpt_goldens.py OUT_DIR

Twelve trainer states — {plain, tied} x {no solver state, velocity, Adam} x {without, with running BatchNorm statistics} — of the smallest
network the tests use with padded channels, every value chosen on the host (set_param, set_solver + set_velocity, set_adam + set_moments,
set_bn_tracking + set_bn_stats).  No training step runs, so the bytes are deterministic.  build_state() is also what the test uses to
rebuild the same states with the code under test."""
import os
import sys

import numpy as np

CASE = (3, 1, 8, 3, 3, 2, 10, 2)          # K, L, FC, W, H, F, A, B: the README tic-tac-toe net with one block
SOLVER = {"velocity": (0.75, 1e-4, 0.5), "adam": (0.0, 1e-4, 0.5), "none": (0.0, 0.0, 0.0)}
ADAM = (0.8, 0.99, 1e-6)
BN_MOMENTUM = 0.9
STATES = [(tied, state, bn) for tied in (False, True) for state in ("none", "velocity", "adam") for bn in (False, True)]


def name(tied, state, bn):
    return "%s_%s%s.agz" % ("tied" if tied else "plain", state, "_bn" if bn else "")


def values(n, salt):
    """n exactly representable floats, distinct within a tensor for the sizes here and different for every (tensor, salt)"""
    return (((np.arange(n, dtype=np.int64) * 37 + salt * 101) % 1021) - 510).astype(np.float32) / np.float32(64)


def bn_values(t, bi):
    C = t.bn_channels(bi)
    return values(C, 900 + bi) / np.float32(8), np.abs(values(C, 950 + bi)) + np.float32(0.25), 1.5 + 0.25 * bi


def build_state(A, ctx, tied, state, bn, salt=0):
    """a trainer in the named state; salt != 0 gives different values everywhere (a trainer to load a fixture INTO)"""
    t = A.Trainer(ctx, *CASE, tied=tied)
    for i in range(t.num_params()):
        t.set_param(i, values(t.param_info(i)[1], salt + i))
    t.set_solver(*SOLVER[state])
    if state == "velocity":
        for i in range(t.num_params()):
            t.set_velocity(i, values(t.param_info(i)[1], salt + 300 + i))
    if state == "adam":
        t.set_adam(*ADAM)
        for i in range(t.num_params()):
            n = t.param_info(i)[1]
            t.set_moments(i, values(n, salt + 500 + i), np.abs(values(n, salt + 700 + i)))
    if bn:
        t.set_bn_tracking(True, BN_MOMENTUM)
        for bi in range(t.num_bn()):
            m, v, w = bn_values(t, bi)
            t.set_bn_stats(bi, m + np.float32(salt), v, w)
    return t


def main(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import agogo_amd as A
    os.makedirs(out, exist_ok=True)
    ctx = A.Ctx(0)
    for tied, state, bn in STATES:
        t = build_state(A, ctx, tied, state, bn)
        t.save(os.path.join(out, name(tied, state, bn)))
        t.close()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
