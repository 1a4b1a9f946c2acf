"""CPU: the packed plane layout of a replay window (agogo_amd/csrc/replay_pack.hpp), on the code the pack and sampler kernels compile.

replay_pack.hpp is the one definition host and device share: k_replay_pack_check / k_replay_pack / k_replay_sample_packed (replay.hip),
agz_replay_pack_host and agz_replay_get.  It includes nothing from HIP, so tests/cpp/replay_pack_check.cpp runs it under g++ -Wall -Werror
and prints the geometry and the packed words of fixed rows; here they are recomputed with Python integers from the declared definition:

    palette        1 to 4 pairwise distinct 32-bit patterns, compared as uint32 (+0.0 and -0.0 differ, a NaN pattern is an entry)
    code           the index of a cell's pattern in the palette; 2 bits a cell, 16 cells a uint32 word
    wpp(mm)        (mm + 15) // 16 words per plane, every plane starts a word
    cell c of plane f of a row     word f * wpp + (c >> 4), bits [2 * (c & 15), +2); unused high bits zero

and the same through libagz (agz_replay_pack_host and agz_encoder_palette need no context).  Planes are compared as uint32 views
everywhere: as floats -0.0 == 0.0, which is the one thing that makes the packing lossless."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
MMS = (1, 9, 15, 16, 17, 25, 42, 361)
PZ, NZ, ONE, MONE, MILLI, NAN1 = 0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3A83126F, 0x7FC00001
PALETTES = ([PZ, NZ, ONE, MONE], [MILLI, PZ, ONE, MONE], [ONE], [MILLI, ONE, MONE], [NZ, NAN1])


def wpp_py(mm):
    return (mm + 15) // 16


def pack_py(codes, F, mm):
    """the words of one row from its cell codes [F * mm], by the definition above"""
    w = wpp_py(mm)
    words = [0] * (F * w)
    for f in range(F):
        for c in range(mm):
            words[f * w + (c >> 4)] |= codes[f * mm + c] << (2 * (c & 15))
    return words


def as_floats(bits):
    return np.array(bits, np.uint32).view(np.float32)


def pack_host_raw(planes, n, F, cells, palette, want_words=True):
    """agz_replay_pack_host as it is: (return code, words or None, first_bad)"""
    L = capi.lib()
    p = np.ascontiguousarray(planes, np.float32)
    pal = np.ascontiguousarray(palette, np.float32)
    words = np.full(n * F * wpp_py(cells), 0xFFFFFFFF, np.uint32) if want_words else None
    bad = C.c_int64(-7)
    r = L.agz_replay_pack_host(capi._pf(p), n, F, cells, capi._pf(pal), len(pal),
                               words.ctypes.data_as(C.POINTER(C.c_uint32)) if want_words else None, C.byref(bad))
    return r, words, bad.value


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay_pack") / "replay_pack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "replay_pack_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REPLAY PACK OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout.splitlines()


def fixed_rows(lines):
    rows, codes, words = {}, {}, {}
    for line in lines:
        w = line.split()
        if w[0] == "row":
            rows[int(w[1])] = (int(w[2]), int(w[3]), int(w[4]), [int(x) for x in w[5:]])
        elif w[0] == "codes":
            codes[int(w[1])] = [int(x) for x in w[2:]]
        elif w[0] == "words":
            words[int(w[1])] = [int(x) for x in w[2:]]
    return rows, codes, words


def test_the_header_under_plain_gxx_against_python(check_output):
    geom = {int(l.split()[1]): int(l.split()[2]) for l in check_output if l.startswith("geom ")}
    assert geom == {mm: wpp_py(mm) for mm in MMS}
    assert geom[361] == 23 and geom[16] == 1 and geom[17] == 2
    cells = [tuple(int(x) for x in l.split()[1:]) for l in check_output if l.startswith("cell ")]
    assert len(cells) == 3 * sum(MMS)
    for mm, f, c, word, shift in cells:
        assert word == f * wpp_py(mm) + (c >> 4) and shift == 2 * (c & 15), (mm, f, c, word, shift)
    rows, codes, words = fixed_rows(check_output)
    assert len(rows) == len(PALETTES) * len(MMS) and set(rows) == set(codes) == set(words)
    seen = set()
    for i, (F, mm, n, pal) in rows.items():
        assert pal == PALETTES[i // len(MMS)] and n == len(pal) and mm == MMS[i % len(MMS)]
        assert len(codes[i]) == F * mm and set(codes[i]) <= set(range(n))
        if F * mm >= 27:
            assert set(codes[i]) == set(range(n)), "the fixed row does not use its whole palette"
        assert words[i] == pack_py(codes[i], F, mm), (i, F, mm)
        seen.add((tuple(pal), mm))
    assert len(seen) == len(PALETTES) * len(MMS)


def test_pack_host_gives_the_words_of_the_definition(check_output):
    rows, codes, words = fixed_rows(check_output)
    for i, (F, mm, n, pal) in rows.items():
        bits = np.array(pal, np.uint32)[np.array(codes[i])]
        r, got, bad = pack_host_raw(bits.view(np.float32), 1, F, mm, as_floats(pal))
        assert r == 0 and bad == -1, (i, capi.lib().agz_last_error())
        assert got.tolist() == words[i], (i, F, mm)
        if mm % 16:                                                    # the unused high bits of every plane's last word are zero
            last = got.reshape(F, wpp_py(mm))[:, -1]
            assert not (last >> np.uint32(2 * (mm % 16))).any()
        r, _, bad = pack_host_raw(bits.view(np.float32), 1, F, mm, as_floats(pal), want_words=False)     # words = NULL: validate only
        assert r == 0 and bad == -1


@pytest.mark.parametrize("pal", PALETTES, ids=["wq", "twoplane", "one-entry", "three-entries", "negzero-nan"])
def test_round_trip_of_several_rows(pal):
    """n rows through agz_replay_pack_host (and the capi wrapper), decoded with Python integers: the input bytes"""
    rng = np.random.default_rng(len(pal))
    for F, mm, n in ((2, 9, 5), (3, 16, 4), (3, 25, 3), (18, 361, 2)):
        bits = rng.choice(np.array(pal, np.uint32), size=(n, F * mm))
        words, bad = capi.replay_pack_host(bits.view(np.float32), F, mm, as_floats(pal))
        assert bad == -1 and words.shape == (n, F * wpp_py(mm)) and words.dtype == np.uint32
        w = wpp_py(mm)
        c = np.arange(mm)
        back = np.zeros_like(bits)
        for f in range(F):
            code = (words[:, f * w + (c >> 4)] >> (2 * (c & 15)).astype(np.uint32)) & 3
            back[:, f * mm:(f + 1) * mm] = np.array((pal + [0] * 4)[:4], np.uint32)[code]
        assert back.tobytes() == bits.tobytes(), (F, mm)
        for row in range(n):                                           # every row starts at its own F * wpp words
            assert words[row].tolist() == pack_py([pal.index(int(b)) for b in bits[row]], F, mm)


def test_the_first_bad_cell_is_the_smallest_linear_index():
    pal = [PZ, NZ, ONE, MONE]
    F, mm, n = 3, 25, 4
    rng = np.random.default_rng(5)
    bits = rng.choice(np.array(pal, np.uint32), size=(n, F * mm))
    bad_bits = bits.copy()
    for row, e in ((3, 2), (1, 60), (1, 31), (2, 0)):
        bad_bits[row, e] = MILLI
    r, words, bad = pack_host_raw(bad_bits.view(np.float32), n, F, mm, as_floats(pal))
    assert r == INVALID and bad == 1 * F * mm + 31
    msg = capi.lib().agz_last_error()
    assert b"row 1" in msg and b"element 31" in msg and b"0x3A83126F" in msg, msg
    assert (words == 0xFFFFFFFF).all()                                 # nothing was written
    r, _, bad = pack_host_raw(bad_bits.view(np.float32), n, F, mm, as_floats(pal), want_words=False)
    assert r == INVALID and bad == 1 * F * mm + 31
    words, bad = capi.replay_pack_host(bad_bits.view(np.float32), F, mm, as_floats(pal))
    assert words is None and bad == 1 * F * mm + 31
    # the very first and the very last element
    for e in (0, n * F * mm - 1):
        b = bits.copy()
        b.reshape(-1)[e] = NAN1
        assert capi.replay_pack_host(b.view(np.float32), F, mm, as_floats(pal), validate_only=True) == (None, e)
    assert capi.replay_pack_host(bits.view(np.float32), F, mm, as_floats(pal), validate_only=True) == (None, -1)


def test_negative_zero_is_not_positive_zero():
    F, mm = 1, 9
    planes = np.zeros((1, F * mm), np.float32)
    planes[0, 4] = -0.0
    assert planes.view(np.uint32)[0, 4] == NZ
    r, _, bad = pack_host_raw(planes, 1, F, mm, as_floats([PZ]))
    assert r == INVALID and bad == 4                                   # -0.0 is out of a palette that holds only +0.0
    r, words, bad = pack_host_raw(planes, 1, F, mm, as_floats([PZ, NZ]))
    assert r == 0 and bad == -1 and words.tolist() == [1 << 8]
    # a NaN entry is matched by its bits: another NaN is not in the palette
    planes.view(np.uint32)[0, 4] = NAN1
    assert pack_host_raw(planes, 1, F, mm, as_floats([PZ, NAN1]))[0] == 0
    assert pack_host_raw(planes, 1, F, mm, as_floats([PZ, 0x7FC00000]))[::2] == (INVALID, 4)


def test_bad_palettes_are_refused():
    L = capi.lib()
    planes = np.zeros((1, 9), np.float32)
    for pal in ([], [0.0, 1.0, -1.0, 0.001, 2.0]):
        p = np.array(pal + [0.0], np.float32)
        assert L.agz_replay_pack_host(capi._pf(planes), 1, 1, 9, capi._pf(p), len(pal), None, None) == INVALID      # n_palette 0 and 5
        assert b"palette" in L.agz_last_error()
    for pal in ([0.0, 1.0, 0.0], [1.0, 1.0], [0.0, -0.0, 1.0, -0.0]):
        assert pack_host_raw(planes, 1, 1, 9, np.array(pal, np.float32))[0] == INVALID                               # duplicates
        assert b"same bit pattern" in L.agz_last_error()
    assert pack_host_raw(planes, 1, 1, 9, np.array([0.0, -0.0], np.float32))[0] == 0      # +0.0 and -0.0 are two entries
    assert L.agz_replay_pack_host(capi._pf(planes), 1, 1, 9, None, 2, None, None) == INVALID
    p = np.array([0.0], np.float32)
    assert L.agz_replay_pack_host(None, 1, 1, 9, capi._pf(p), 1, None, None) == INVALID
    assert L.agz_replay_pack_host(capi._pf(planes), 1, 0, 9, capi._pf(p), 1, None, None) == INVALID
    assert L.agz_replay_pack_host(None, 0, 1, 9, capi._pf(p), 1, None, None) == 0         # no rows: nothing to do
    # the packed create refuses a bad palette (and a NULL context) before it touches a device
    out = C.c_void_p()
    pal = np.array([0.0, 1.0], np.float32)
    assert L.agz_replay_create_packed(None, 2, 3, 3, 10, 5, capi._pf(pal), 2, C.byref(out)) == INVALID
    assert b"NULL" in L.agz_last_error()
    assert L.agz_replay_storage(None, None, None, None) == INVALID


def test_encoder_palettes_are_the_literals_the_encoders_write():
    wq = capi.encoder_palette(capi.ENC_WQ)
    assert wq.dtype == np.float32 and wq.view(np.uint32).tolist() == [PZ, NZ, ONE, MONE]
    tp = capi.encoder_palette(capi.ENC_TWOPLANE)
    assert tp.view(np.uint32).tolist() == [MILLI, PZ, ONE, MONE]
    assert tp.tobytes() == np.array([0.001, 0.0, 1.0, -1.0], np.float32).tobytes()
    L = capi.lib()
    pal, n = (C.c_float * 4)(), C.c_int32(0)
    assert L.agz_encoder_palette(7, pal, C.byref(n)) == INVALID
    assert b"unknown encoder" in L.agz_last_error()
    assert L.agz_encoder_palette(-1, pal, C.byref(n)) == INVALID
    assert L.agz_encoder_palette(capi.ENC_WQ, None, C.byref(n)) == INVALID
    with pytest.raises(capi.AgzError):
        capi.encoder_palette(2)
