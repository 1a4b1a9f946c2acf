"""GPU: agz_replay_save / agz_replay_load — a saved window continues bit for bit (include/agz.h, DESIGN.md §2 `replay-ckpt`;
k_replay_ckpt_scan, k_replay_ckpt_put and the chunked streaming of replay.hip).

Every comparison is of bytes (`.tobytes()`), never of floats: -0.0, +0.0 and a NaN pattern are in the palettes the planes are drawn from
(PALETTES and make_rows of test_replay_packed_gpu.py).  Nothing here takes a tolerance.  The windows are toys: capacity 7 fed 10 rows by
the three append routes, so the ring has wrapped and its head is at slot 3, and the staging buffers hold 3 rows of planes, so the chunks
cut inside every array and the wrap falls inside a chunk.  F = 2 on 5x5 (a plane's second word has fourteen unused bits) and on 4x4 (a
plane is exactly one word), F = 3 on 3x5 (not square: sampled with symmetric = 0 only), and F = 2 on 3x3, the shape of
test_replay_gpu.py's trainers.  The expected file is the `struct` restatement of test_replay_ckpt_cpu.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import agogo_amd as A
from agogo_amd import capi
import test_replay_sharded_gpu as S
from test_replay_ckpt_cpu import digest_py, file_bytes
from test_replay_gpu import _trainers
from test_replay_packed_gpu import PALETTES, Feeder, make_rows, pal_floats, same

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4
CAP, FED = 7, 10
SHAPES = {"5x5": (2, 5, 5, 26), "4x4": (2, 4, 4, 17), "3x5": (3, 3, 5, 16), "3x3": (2, 3, 3, 10)}     # F, H, W, PolicyLen
FORMS = ("fp32", "packed")


def plane_bytes(shape, packed):
    F, H, W, _ = shape
    return 4 * F * ((H * W + 15) // 16 if packed else H * W)


def window(ctx, shape, cap, packed, pal, staging_rows_of=None):
    """a window whose staging holds 3 rows of planes — its own, or those of a file of the other form it is about to load"""
    rp = A.Replay(ctx, *shape, cap, palette=pal_floats(pal) if packed else None)
    rp.set_ckpt_staging(3 * plane_bytes(shape, packed if staging_rows_of is None else staging_rows_of))
    return rp


def source(ctx, shape, packed, pal, seed=1, cap=CAP, also=()):
    """a window of `cap` slots fed FED rows by the three append routes (and every window of `also` with it), with its feeder"""
    rp = window(ctx, shape, cap, packed, pal)
    fd = Feeder(ctx, [rp, *also], np.random.default_rng(seed), pal)
    for n in (4, 3, 3):
        fd.append(n)
    assert rp.total() == FED and len(rp) == min(FED, cap)
    return rp, fd


def state(rp, samples=True):
    """everything a window shows: counts, rows, digest and two minibatches (symmetric where the board is square), as bytes"""
    out = [len(rp), rp.total(), rp.digest()] + [a.tobytes() for a in rp.get()]
    if samples and len(rp):
        for step in (0, 3):
            out += [a.tobytes() for a in rp.sample(8, 77, step, rp.H == rp.W)]
    return out


def header(path):
    b = open(path, "rb").read()
    return dict(zip(("total", "live", "capacity", "digest"), struct.unpack_from("<4Q", b, 48)))


def load_rc(rp, path):
    rc = capi.lib().agz_replay_load(rp.h, os.fsencode(str(path)))
    return rc, capi.lib().agz_last_error().decode()


@pytest.mark.parametrize("pal", list(PALETTES))
@pytest.mark.parametrize("shape", ["5x5", "4x4", "3x5"])
def test_round_trip_each_form_each_palette(ctx, tmp_path, shape, pal):
    sh = SHAPES[shape]
    for packed in (False, True):
        src, fd = source(ctx, sh, packed, pal)
        path = str(tmp_path / ("w_%d.rpw" % packed))
        before = state(src)
        src.save(path)
        assert state(src) == before                                       # a save does not change the window
        dst = window(ctx, sh, CAP, packed, pal)
        dst.load(path)
        assert len(dst) == CAP and dst.total() == FED
        assert all(same(a, b) for a, b in zip(dst.get(0, len(dst)), src.get(0, len(src))))
        assert dst.digest() == src.digest() == header(path)["digest"] == digest_py(*fd.live())
        sym = sh[1] == sh[2]
        assert all(same(a, b) for a, b in zip(dst.sample(8, 77, 3, sym), src.sample(8, 77, 3, sym)))
        assert state(dst) == before
        want = file_bytes(sh, *fd.live(), FED, CAP, palette=PALETTES[pal] if packed else None)
        assert open(path, "rb").read() == want, "the file is not what replay_ckpt.hpp's comment says"
        assert not os.path.exists(path + ".tmp")
        for h in (fd, src, dst):
            h.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ["5x5", "4x4", "3x5", "3x3"])
def test_a_loaded_window_continues_as_the_one_never_saved(ctx, tmp_path, shape, form):
    sh, pal, packed = SHAPES[shape], "twoplane", form == "packed"
    src, fd = source(ctx, sh, packed, pal)
    path = str(tmp_path / "w.rpw")
    src.save(path)
    dst = window(ctx, sh, CAP, packed, pal)
    dst.load(path)
    fd.windows = [src, dst]
    for n in (1, 2, 3):                                                   # 6 more rows into both, by the three routes
        fd.append(n)
        assert state(dst) == state(src)
    assert dst.total() == FED + 6
    p, q, v = fd.live()
    assert all(same(a, b) for a, b in zip(dst.get(), (p, q, v)))
    if shape == "3x3":                                                    # the shape of test_replay_gpu.py's trainers
        for adam in (False, True):
            ta, tb = _trainers(ctx, 2, adam)
            ca, cb = ta.train_replay(src, 3, 4242, True), tb.train_replay(dst, 3, 4242, True)
            assert np.float32(ca).tobytes() == np.float32(cb).tobytes(), (adam, ca, cb)
            fresh, = _trainers(ctx, 1, adam)
            changed = False
            for i in range(ta.num_params()):
                assert ta.get_param(i).tobytes() == tb.get_param(i).tobytes(), (adam, ta.param_info(i))
                changed = changed or ta.get_param(i).tobytes() != fresh.get_param(i).tobytes()
            assert changed                                                # training changed the parameters
            for t in (ta, tb, fresh):
                t.close()
    for h in (fd, src, dst):
        h.close()


@pytest.mark.parametrize("form", FORMS)
def test_the_smallest_staging_one_row_a_chunk(ctx, tmp_path, form):
    """4 bytes of staging, the floor, on the smallest shape: every chunk of every array is one row, through the wrap of the ring"""
    sh, pal, packed = SHAPES["3x3"], "twoplane", form == "packed"
    src, fd = source(ctx, sh, packed, pal)                                # capacity 7 fed 10 rows: the oldest live row lies in slot 3
    src.set_ckpt_staging(4)
    path = str(tmp_path / "floor.rpw")
    before = state(src)
    src.save(path)
    assert state(src) == before
    assert open(path, "rb").read() == file_bytes(sh, *fd.live(), FED, CAP, palette=PALETTES[pal] if packed else None)
    dst = window(ctx, sh, CAP, packed, pal)
    dst.set_ckpt_staging(4)
    dst.load(path)
    assert state(dst) == before and dst.digest() == header(path)["digest"]
    for h in (fd, src, dst):
        h.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ["5x5", "4x4", "3x5"])
def test_other_capacities(ctx, tmp_path, shape, form):
    sh, pal, packed = SHAPES[shape], "wq", form == "packed"
    big_ref = window(ctx, sh, 12, packed, pal)                            # a capacity-12 window fed the same rows from the start
    src, fd = source(ctx, sh, packed, pal, also=[big_ref])
    path = str(tmp_path / "w.rpw")
    src.save(path)
    p, q, v = fd.live()                                                   # the 7 rows of the file
    big = window(ctx, sh, 12, packed, pal)
    big.load(path)
    assert len(big) == 7 and big.total() == FED and big.capacity == 12   # simply not yet full
    assert all(same(a, b) for a, b in zip(big.get(), (p, q, v))) and big.digest() == src.digest()
    fd.windows = [big, big_ref]
    fd.append(2)                                                          # 9 of 12: the loaded window lacks the three rows the file never held
    assert len(big) == 9 and len(big_ref) == 12 and big.total() == big_ref.total() == FED + 2
    assert all(same(a, b) for a, b in zip(big.get(), [x[-9:] for x in (fd.P, fd.Q, fd.V)]))
    # the not-yet-full window is itself savable: its file loads into capacity 12 and 7 and continues as `big` does
    again = str(tmp_path / "again.rpw")
    big.save(again)
    hd = header(again)
    assert (hd["total"], hd["live"], hd["digest"]) == (FED + 2, 9, big.digest()) and hd["live"] == min(hd["total"], hd["capacity"])
    assert open(again, "rb").read() == file_bytes(sh, *[x[-9:] for x in (fd.P, fd.Q, fd.V)], FED + 2, hd["capacity"],
                                                  palette=PALETTES[pal] if packed else None)
    big2, seven, seven_ref = window(ctx, sh, 12, packed, pal), window(ctx, sh, CAP, packed, pal), window(ctx, sh, CAP, packed, pal)
    big2.load(again)
    seven.load(again)
    seven_ref.append_host(*[x[:FED + 2] for x in (fd.P, fd.Q, fd.V)])
    assert state(big2) == state(big) and state(seven) == state(seven_ref) and len(seven) == CAP and seven.total() == FED + 2
    fd.windows = [big, big_ref, big2, seven, seven_ref]
    for n in (3, 1, 4):                                                   # full at 10 + 5 rows; from there on it is the window fed from the start
        fd.append(n)
        assert state(big) == state(big_ref), n
        assert state(big2) == state(big) and state(seven) == state(seven_ref), n
    assert big.total() == FED + 10
    small = window(ctx, sh, 4, packed, pal)
    small.load(path)
    assert len(small) == 4 and small.total() == FED                       # the newest 4 rows, as after one long append
    assert all(same(a, b) for a, b in zip(small.get(), (p[-4:], q[-4:], v[-4:])))
    small_ref = window(ctx, sh, 4, packed, pal)
    small_ref.append_host(*[x[:FED] for x in (fd.P, fd.Q, fd.V)])
    fd.windows = [small, small_ref]
    assert state(small) == state(small_ref)
    fd.append(3)
    assert state(small) == state(small_ref)
    for h in (fd, src, big, big_ref, big2, seven, seven_ref, small, small_ref):
        h.close()


@pytest.mark.parametrize("shape", ["5x5", "4x4", "3x5"])
def test_cross_form_loads_convert_on_the_device(ctx, tmp_path, shape):
    sh, pal = SHAPES[shape], "three"
    xs = sh[0] * sh[1] * sh[2]
    files, rows = {}, None
    for packed in (False, True):
        src, fd = source(ctx, sh, packed, pal, seed=5)
        files[packed] = str(tmp_path / ("w_%d.rpw" % packed))
        src.save(files[packed])
        rows, digest = fd.live(), src.digest()
        fd.close()
        src.close()
    for packed in (False, True):                                          # the file's form; the window has the other one
        dst = window(ctx, sh, CAP, not packed, pal, staging_rows_of=packed)
        dst.load(files[packed])
        assert len(dst) == CAP and dst.total() == FED and dst.digest() == digest
        assert all(same(a, b) for a, b in zip(dst.get(), rows))
        assert dst.storage()[0] is (not packed)
        dst.close()
    # packed -> packed under a permuted, larger palette: the codes are remapped through the patterns
    perm = [PALETTES[pal][2], 0x12345678, PALETTES[pal][0], PALETTES[pal][1]]
    dst = A.Replay(ctx, *sh, CAP, palette=np.array(perm, np.uint32).view(np.float32))
    dst.set_ckpt_staging(3 * plane_bytes(sh, True))
    dst.load(files[True])
    assert all(same(a, b) for a, b in zip(dst.get(), rows)) and dst.digest() == digest
    x, _, _ = dst.sample(8, 5, 1, False)
    assert set(np.unique(x.view(np.uint32)).tolist()) <= set(PALETTES[pal])
    keep = state(dst)
    # a packed file whose palette has an entry the window's lacks
    lacks = A.Replay(ctx, *sh, CAP, palette=np.array(PALETTES[pal][:2], np.uint32).view(np.float32))
    lacks.append_host(*make_rows(np.random.default_rng(2), 2, *sh, "one")[:1], *[a[:2] for a in rows[1:]])
    before = state(lacks)
    rc, msg = load_rc(lacks, files[True])
    assert rc == INVALID and "0x%08X" % PALETTES[pal][2] in msg and "palette" in msg, msg
    assert state(lacks) == before
    # an fp32 file with two cells outside the window's palette: the refusal names the smaller one
    b = bytearray(open(files[False], "rb").read())
    for row, el, bits in ((5, 3, 0x40000000), (2, xs - 1, 0x40400000)):
        struct.pack_into("<I", b, 80 + 4 * (row * xs + el), bits)
    planes = np.frombuffer(bytes(b[80:80 + 4 * CAP * xs]), np.uint32).reshape(CAP, xs)
    struct.pack_into("<Q", b, 72, digest_py(planes, rows[1], rows[2]))    # (the digest is right: only the palette is at fault)
    bad = str(tmp_path / "outside.rpw")
    open(bad, "wb").write(bytes(b))
    rc, msg = load_rc(dst, bad)
    assert rc == INVALID and "row 2, element %d " % (xs - 1) in msg and "0x40400000" in msg, msg
    assert state(dst) == keep
    plain = window(ctx, sh, CAP, False, pal)                              # an fp32 window takes the same file: any pattern is a float
    plain.load(bad)
    assert plain.get()[0].view(np.uint32)[2, xs - 1] == 0x40400000
    for h in (dst, lacks, plain):
        h.close()


def _patched(tmp_path, name, good, edit):
    b = bytearray(open(good, "rb").read())
    b = edit(b) or b
    path = str(tmp_path / name)
    open(path, "wb").write(bytes(b))
    return path


@pytest.mark.parametrize("shape", ["5x5", "4x4", "3x5"])
def test_a_bad_file_changes_nothing(ctx, tmp_path, shape):
    sh, pal = SHAPES[shape], "three"
    F, H, W, A1 = sh
    mm, wpp = H * W, (H * W + 15) // 16
    good = {}
    for packed in (False, True):
        src, fd = source(ctx, sh, packed, pal, seed=9)
        good[packed] = str(tmp_path / ("good_%d.rpw" % packed))
        src.save(good[packed])
        fd.close()
        src.close()
    for packed in (False, True):
        pb = plane_bytes(sh, packed)
        off_policy, off_value = 80 + CAP * pb, 80 + CAP * pb + CAP * A1 * 4
        target, tfd = source(ctx, sh, packed, pal, seed=10, cap=5)        # holds other rows, at another capacity
        before = state(target)

        def refused(path, *tokens):
            rc, msg = load_rc(target, path)
            assert rc == INVALID, (path, rc, msg)
            for t in tokens:
                assert t in msg, (path, msg)
            assert state(target) == before, path

        def flip(at):
            def edit(b):
                b[at] ^= 0x10
            return edit

        for i, field in enumerate(("Features", "Height", "Width", "PolicyLen")):      # wrong shape: each field, named
            other = list(sh)
            other[i] += 1
            w = A.Replay(ctx, *other, 5, palette=pal_floats(pal) if packed else None)
            rc, msg = load_rc(w, good[packed])
            assert rc == INVALID and field in msg and len(w) == 0 and w.total() == 0, msg
            w.close()
        refused(_patched(tmp_path, "cut", good[packed], lambda b: b[:-1]), "bytes long")
        refused(_patched(tmp_path, "long", good[packed], lambda b: b + b"\0"), "bytes long")
        refused(_patched(tmp_path, "planes", good[packed], flip(80 + 2 * pb + 1)), *(("digest",) if not packed else ()))
        refused(_patched(tmp_path, "policy", good[packed], flip(off_policy + 4 * (3 * A1 + 2))), "digest")
        refused(_patched(tmp_path, "value", good[packed], flip(off_value + 4 * 6 + 3)), "digest")
        refused(_patched(tmp_path, "live", good[packed], lambda b: struct.pack_into("<Q", b, 48, 6)), "> total")
        refused(_patched(tmp_path, "magic", good[packed], lambda b: struct.pack_into("<c", b, 0, b"B")), "magic")
        refused(_patched(tmp_path, "endmark", good[packed], lambda b: struct.pack_into("<c", b, len(b) - 9, b"X")), "end marker")
        refused(str(tmp_path / "nothing.rpw"), "cannot open")
        if packed:
            word = lambda row, f, w: 80 + 4 * ((row * F + f) * wpp + w)
            def code3(b):                                                 # a code 3 in a file of n_palette 3: cell 1 of plane 1 of row 4
                v, = struct.unpack_from("<I", b, word(4, 1, 0))
                struct.pack_into("<I", b, word(4, 1, 0), v | (3 << 2))
            refused(_patched(tmp_path, "code3", good[packed], code3), "row 4, element %d " % (mm + 1), "code 3")
            if mm % 16:
                def high(b):                                              # a set bit past the last cell of plane 0 of row 6
                    v, = struct.unpack_from("<I", b, word(6, 0, wpp - 1))
                    struct.pack_into("<I", b, word(6, 0, wpp - 1), v | (1 << 31))
                refused(_patched(tmp_path, "highbit", good[packed], high), "row 6, plane 0", "past the plane's last cell")
        for h in (target, tfd):
            h.close()


@pytest.mark.parametrize("form", FORMS)
def test_the_save_is_atomic(ctx, tmp_path, form):
    sh, pal, packed = SHAPES["5x5"], "wq", form == "packed"
    L = capi.lib()
    src, fd = source(ctx, sh, packed, pal)
    nowhere = str(tmp_path / "no_such_dir" / "w.rpw")
    assert L.agz_replay_save(src.h, os.fsencode(nowhere)) == INVALID
    assert not os.path.exists(nowhere + ".tmp") and not os.path.exists(os.path.dirname(nowhere))
    path = str(tmp_path / "w.rpw")
    src.save(path)
    first, first_state = open(path, "rb").read(), state(src)
    fd.append(2)
    src.save(path)                                                        # a second save over an existing file replaces it
    second = open(path, "rb").read()
    assert second != first and second == file_bytes(sh, *fd.live(), FED + 2, CAP, palette=PALETTES[pal] if packed else None)
    assert not os.path.exists(path + ".tmp")
    fd.append(1)
    os.mkdir(path + ".tmp")                                               # a save of this very path fails (its temporary file cannot be opened) ...
    assert L.agz_replay_save(src.h, os.fsencode(path)) == INVALID
    os.rmdir(path + ".tmp")
    assert open(path, "rb").read() == second                              # ... and the earlier file is intact and still loads
    dst = window(ctx, sh, CAP, packed, pal)
    dst.load(path)
    assert len(dst) == CAP and dst.total() == FED + 2 and dst.digest() == header(path)["digest"] != src.digest()
    src.save(path)
    dst.load(path)
    assert state(dst) == state(src) and state(src) != first_state
    for h in (fd, src, dst):
        h.close()


@pytest.mark.parametrize("form", FORMS)
def test_an_empty_window_saves_and_loads(ctx, tmp_path, form):
    sh, pal, packed = SHAPES["4x4"], "twoplane", form == "packed"
    L = capi.lib()
    empty = window(ctx, sh, CAP, packed, pal)
    path = str(tmp_path / "empty.rpw")
    empty.save(path)
    assert open(path, "rb").read() == file_bytes(sh, np.zeros((0, 32), np.uint32), np.zeros((0, 17), np.uint32), np.zeros(0, np.uint32), 0, CAP,
                                                 palette=PALETTES[pal] if packed else None) and os.path.getsize(path) == 96
    dst, fd = source(ctx, sh, packed, pal)                                # a loaded empty file empties a window that held rows
    dst.load(path)
    assert len(dst) == 0 and dst.total() == 0 and dst.digest() == 0
    x, p, v = np.zeros((1, *sh[:3]), np.float32), np.zeros((1, sh[3]), np.float32), np.zeros(1, np.float32)
    assert L.agz_replay_sample(dst.h, 1, 1, 0, 0, capi._pf(x), capi._pf(p), capi._pf(v)) == STATE
    assert b"empty" in L.agz_last_error()
    fd.windows = [dst, empty]
    fd.append(3)                                                          # and it fills again from slot 0
    assert state(dst) == state(empty) and dst.total() == 3
    for h in (fd, dst, empty):
        h.close()


CKPT_JOBS = r"""
for ji, job in enumerate(jobs):
    K, L, FC, W, H, F, Aspace, Bg = job["conf"]
    steps, seed = job["steps"], job["seed"]
    res = {}
    same_file = A.Replay(ctx, F, H, W, Aspace, job["cap"], palette=np.load(job["palette"]) if job["packed"] else None)
    same_file.set_ckpt_staging(3 * 4 * F * H * W)
    same_file.load(job["good"])                                       # every rank loads one file into its replica
    res["counts"] = np.array([len(same_file), same_file.total()])
    res["digest"] = np.uint64(same_file.digest())
    differs = A.Replay(ctx, F, H, W, Aspace, job["cap"], palette=np.load(job["palette"]) if job["packed"] else None)
    differs.load(job["good"] if rank == 0 else job["other"])          # rank 1's file differs in one row
    for tied in (0, 1):
        tag = "tied_" if tied else "plain_"
        t = make(job, tied, 0)
        before = [t.get_param(i).tobytes() for i in range(t.num_params())]
        res[tag + "msg"] = np.array(err(lambda: t.train_replay_sharded(differs, steps, seed, True, True)))
        res[tag + "untouched"] = np.array(before == [t.get_param(i).tobytes() for i in range(t.num_params())])
        res[tag + "cost"] = np.float32(t.train_replay_sharded(same_file, steps, seed, True, True))
        res[tag + "trained"] = np.array(before != [t.get_param(i).tobytes() for i in range(t.num_params())])
        t.close()
    same_file.close()
    differs.close()
    np.savez(job["out"] % rank, **res)
comm.close()
ctx.close()
"""


@pytest.mark.parametrize("form", FORMS)
def test_every_rank_loads_one_file_into_its_replica(ctx, tmp_path, monkeypatch, form):
    """two ranks (processes on GPU 0 through tests/fake_rccl, the helpers of test_replay_sharded_gpu.py) load one file: the digests agree
    and agz_train_replay_sharded(verify = 1) trains; with rank 1 loading a file that differs in one row it is AGZ_E_STATE on every rank"""
    K, blocks, FC, W, H, F, Aspace, Bg = S.CONF
    sh, pal, packed = (F, H, W, Aspace), "twoplane", form == "packed"
    src, fd = source(ctx, sh, packed, pal, cap=S.TRAIN_CAP)
    fd.append(9)                                                          # 19 rows into 12 slots: wrapped
    good, other, palette = str(tmp_path / "good.rpw"), str(tmp_path / "other.rpw"), str(tmp_path / "palette.npy")
    src.save(good)
    p, q, v = (a.copy() for a in fd.live())
    q[-2, 3] = np.nextafter(q[-2, 3], np.float32(9))                      # one policy value of one row
    twin = window(ctx, sh, S.TRAIN_CAP, packed, pal)
    twin.append_host(p[:7], q[:7], v[:7])
    twin.append_host(p, q, v)                                             # the same counts: total 19, live 12
    twin.save(other)
    assert header(other)["total"] == header(good)["total"] == FED + 9 and header(other)["digest"] != header(good)["digest"]
    np.save(palette, pal_floats(pal))
    job = {"conf": S.CONF, "cap": S.TRAIN_CAP, "steps": S.STEPS, "seed": S.SEED, "good": good, "other": other, "palette": palette, "packed": packed}
    monkeypatch.setattr(S, "WORKER", S.WORKER.split("for ji, job in enumerate(jobs):")[0] + CKPT_JOBS)
    R = S.run_ranks(2, [job], tmp_path, "ckpt")[0]
    for r in range(2):
        assert R[r]["counts"].tolist() == [S.TRAIN_CAP, FED + 9] and int(R[r]["digest"]) == src.digest()
        for tag in ("plain_", "tied_"):
            msg = str(R[r][tag + "msg"])
            assert "(%d)" % STATE in msg and "rank 1" in msg and "digest" in msg, (tag, r, msg)
            assert bool(R[r][tag + "untouched"]) and bool(R[r][tag + "trained"]) and np.isfinite(float(R[r][tag + "cost"]))
    for tag in ("plain_", "tied_"):
        assert R[0][tag + "cost"].tobytes() == R[1][tag + "cost"].tobytes()
    for h in (fd, src, twin):
        h.close()
