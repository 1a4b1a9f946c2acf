"""CPU: the replay window's checkpoint format, checked on the code the window runs.

agogo_amd/csrc/replay_ckpt.hpp is the only place that knows the bytes of an agz_replay_save file and the only place that validates its
header and lengths.  It includes nothing from HIP, so tests/cpp/replay_ckpt_check.cpp runs it under g++ on a toy window (F = 2 on a 5x5
board: 25 cells, two words a plane with fourteen unused bits in the second; PolicyLen 26; total 10, live 7, capacity 7) in both forms,
written and read in chunks of 3 rows: the round trip, EVERY truncation, a trailing byte, and one corruption per rule read_head()
enforces.  The bytes themselves are rebuilt here with `struct` from the format comment of the header (file_bytes, which
tests/test_replay_ckpt_gpu.py uses too), so the comment and the code cannot drift; the digest in the header is replay.hpp's, restated here
with Python integers and compared with agz_replay_digest_host.  The same program holds the header's chunk planner (row_chunks), by which
replay.hip streams the arrays, to its contract."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np

from agogo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join("tests", "cpp", "replay_ckpt_check.cpp")
HEADER = os.path.join("agogo_amd", "csrc", "replay_ckpt.hpp")
M64 = (1 << 64) - 1
F, H, W, A1, TOTAL, LIVE, CAP = 2, 5, 5, 26, 10, 7, 7
PAL = [0x00000000, 0x80000000, 0x3F800000, 0x7FC00001]                 # +0.0, -0.0, 1.0 and a NaN pattern


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_py(planes, policy, value):
    """replay.hpp's digest of n rows of bit patterns in logical order: n + the sum of mix64(mix64(j * rowlen + e) ^ bits(j, e))"""
    planes, policy, value = (np.ascontiguousarray(a).view(np.uint32) for a in (planes, policy, value))
    n = value.size
    rows = np.concatenate([planes.reshape(n, -1), policy.reshape(n, -1), value.reshape(n, 1)], axis=1) if n else np.zeros((0, 1), np.uint32)
    rowlen = rows.shape[1]
    d = n
    for j in range(n):
        for e in range(rowlen):
            d = (d + mix64(mix64(j * rowlen + e) ^ int(rows[j, e]))) & M64
    return d


def pack_py(planes, Features, cells, palette):
    """replay_pack.hpp's layout: cell c of plane f in word f * wpp + (c >> 4), bits [2 (c & 15), 2 (c & 15) + 2); unused bits zero"""
    planes = np.ascontiguousarray(planes).view(np.uint32).reshape(-1, Features, cells)
    wpp = (cells + 15) // 16
    words = np.zeros((planes.shape[0], Features * wpp), np.uint32)
    for j in range(planes.shape[0]):
        for f in range(Features):
            for c in range(cells):
                words[j, f * wpp + (c >> 4)] |= np.uint32(palette.index(int(planes[j, f, c])) << (2 * (c & 15)))
    return words


def file_bytes(shape, planes, policy, value, total, capacity, palette=None, digest=None):
    """the file of a window, from the format comment of replay_ckpt.hpp: `planes` [live][F * H * W], `policy` [live][PolicyLen], `value`
    [live] are the LIVE rows in logical order; palette (a list of bit patterns) makes it a packed file"""
    Features, Height, Width, PolicyLen = shape
    planes, policy, value = (np.ascontiguousarray(a).view(np.uint32) for a in (planes, policy, value))
    live = value.size
    assert live == min(total, capacity)
    b = b"AGZRPW01"
    b += struct.pack("<4I", Features, Height, Width, PolicyLen)                                        # shape
    pal = list(palette or [])
    b += struct.pack("<2I4I", 1 if palette else 0, len(pal), *(pal + [0] * (4 - len(pal))))            # form, n_palette, palette[4]
    b += struct.pack("<3Q", total, live, capacity)                                                     # counts
    b += struct.pack("<Q", digest_py(planes, policy, value) if digest is None else digest)             # digest
    body = pack_py(planes, Features, Height * Width, pal) if palette else planes
    b += body.astype("<u4").tobytes() + policy.astype("<u4").tobytes() + value.astype("<u4").tobytes() # planes, policy, value
    return b + b"AGZRPWZZ" + struct.pack("<Q", len(b) + 16)                                            # end


def toy_rows():
    planes = np.array([[PAL[(j * 7 + f * 3 + c * 5 + (c >> 2)) & 3] for f in range(F) for c in range(H * W)] for j in range(LIVE)], np.uint32)
    policy = np.array([[0x3C000000 + j * 1000 + e for e in range(A1)] for j in range(LIVE)], np.uint32)
    value = np.array([0xBF000000 + j for j in range(LIVE)], np.uint32)
    return planes, policy, value


def run_check(root, tmp_path, extra=()):
    """compile the check against the header under `root`, run it, compare the files it wrote; the first thing that is wrong, or None"""
    exe, out_dir = str(tmp_path / "replay_ckpt_check"), tmp_path / "files"
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(root, CHECK)])
    out = subprocess.run([exe, str(out_dir)], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 or "REPLAY CKPT OK" not in out.stdout:
        return "the check failed:\n" + out.stdout[-3000:] + out.stderr[-3000:]
    planes, policy, value = toy_rows()
    if int(re.search(r"^digest (\d+)$", out.stdout, re.M).group(1)) != digest_py(planes, policy, value):
        return "the digest of the toy rows moved"
    if open(out_dir / "toy_fp32.bin", "rb").read() != file_bytes((F, H, W, A1), planes, policy, value, TOTAL, CAP):
        return "the bytes of the fp32 toy file moved"
    if open(out_dir / "toy_packed.bin", "rb").read() != file_bytes((F, H, W, A1), planes, policy, value, TOTAL, CAP, palette=PAL):
        return "the bytes of the packed toy file moved"
    return None


def test_the_codec_writes_the_documented_bytes_and_refuses_every_bad_header(tmp_path):
    assert run_check(ROOT, tmp_path) is None


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone program again, instrumented: every truncated and corrupted file walks read_head()'s reads and seeks"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    linked = subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    assert linked.returncode == 0, "this g++ does not link the sanitizer runtimes, so the instrumented run cannot be made:\n" + linked.stderr[-2000:]
    assert run_check(ROOT, tmp_path, extra=flags) is None


def test_the_header_digest_is_the_library_digest_of_the_same_rows():
    planes, policy, value = toy_rows()
    want = digest_py(planes, policy, value)
    assert capi.replay_digest_host(planes.view(np.float32), policy.view(np.float32), value.view(np.float32), F, H * W, A1) == want
    for pal in (None, PAL):
        b = file_bytes((F, H, W, A1), planes, policy, value, TOTAL, CAP, palette=pal)
        assert struct.unpack_from("<Q", b, 72)[0] == want and len(b) == 96 + LIVE * ((16 if pal else 200) + 104 + 4)
    assert digest_py(planes[:0], policy[:0], value[:0]) == 0


def test_a_mutated_header_fails_the_check(tmp_path):
    """the check is not vacuous: two runs swapped, a rule of read_head() dropped or weakened, a file that may run on, a planner that breaks
    its contract — each is caught by the program or by the byte comparison"""
    hdr = open(os.path.join(ROOT, HEADER)).read()
    muts = [("const uint64_t counts[4] = {h.total, h.live, h.capacity, h.digest};", "const uint64_t counts[4] = {h.live, h.total, h.capacity, h.digest};"),
            ("if ((uint64_t)len != l.total)", "if ((uint64_t)len < l.total)"), ("if (h.live > h.total)", "if (false)"),
            ("h.live != replay::live(h.total, h.capacity)", "h.live > replay::live(h.total, h.capacity)"),
            ("l.row_bytes[POLICY] = 4ull * h.A1;", "l.row_bytes[POLICY] = 4ull * h.A1 + 4;"), ("if (h.form > 1)", "if (h.form > 2)"),
            ("      if (h.palette[i]) return fail", "      if (false) return fail"), ("|| total != l.total) return fail", ") return fail"),
            ("if (rows < 1) rows = 1;", "if (rows < 1) rows = 0;")]     # the planner: staging below one row no longer gives one row a chunk
    os.makedirs(tmp_path / "agogo_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "cpp")
    shutil.copy(os.path.join(ROOT, CHECK), tmp_path / CHECK)
    for name in ("replay.hpp", "replay_pack.hpp"):
        shutil.copy(os.path.join(ROOT, "agogo_amd", "csrc", name), tmp_path / "agogo_amd" / "csrc" / name)
    for old, new in muts:
        assert hdr.count(old) == 1, old
        (tmp_path / HEADER).write_text(hdr.replace(old, new))
        assert run_check(str(tmp_path), tmp_path) is not None, "mutation %r passes the check" % new
    (tmp_path / HEADER).write_text(hdr)
    assert run_check(str(tmp_path), tmp_path) is None


def test_the_new_symbols_through_every_binding():
    """the ABI: the two calls and the debug hook are declared in the headers, bound by capi.py with their argument types, called by the Go
    shim with as many arguments, mirrored by the C++ host header, and refuse NULL without a device"""
    L = capi.lib()
    INVALID = -1
    agz_h = open(os.path.join(ROOT, "include", "agz.h")).read()
    dbg_h = open(os.path.join(ROOT, "include", "agz_debug.h")).read()
    assert re.search(r"^int agz_replay_save\(agz_replay\* rp, const char\* path\);$", agz_h, re.M)
    assert re.search(r"^int agz_replay_load\(agz_replay\* rp, const char\* path\);$", agz_h, re.M)
    assert re.search(r"^int agz_replay_set_ckpt_staging\(agz_replay\* rp, size_t bytes\);$", dbg_h, re.M)
    for name, argtypes in (("agz_replay_save", [C.c_void_p, C.c_char_p]), ("agz_replay_load", [C.c_void_p, C.c_char_p]),
                           ("agz_replay_set_ckpt_staging", [C.c_void_p, C.c_size_t])):
        fn = getattr(L, name)
        assert fn.restype == C.c_int32 and list(fn.argtypes) == argtypes, name
    assert L.agz_replay_save(None, b"x") == INVALID and b"NULL" in L.agz_last_error()
    assert L.agz_replay_load(None, b"x") == INVALID and b"NULL" in L.agz_last_error()
    assert L.agz_replay_save(None, None) == INVALID and L.agz_replay_load(None, None) == INVALID
    assert L.agz_replay_set_ckpt_staging(None, 64) == INVALID and b"NULL" in L.agz_last_error()
    assert not os.path.exists("x") and not os.path.exists("x.tmp")
    for method in ("save", "load", "set_ckpt_staging"):
        assert callable(getattr(capi.Replay, method))
    go = open(os.path.join(ROOT, "go", "agzhip", "agzhip.go")).read()
    assert re.search(r"func \(r \*Replay\) Save\(path string\) error \{[^}]*C\.agz_replay_save\(r\.h, p\)", go, re.S)
    assert re.search(r"func \(r \*Replay\) Load\(path string\) error \{[^}]*C\.agz_replay_load\(r\.h, p\)", go, re.S)
    host = open(os.path.join(ROOT, "agogo_amd", "host", "agogo.hpp")).read()
    assert "agz_replay_save(h, path.c_str())" in host and "agz_replay_load(h, path.c_str())" in host
    assert "void SaveRun(const std::string& prefix)" in host and "void LoadRun(const std::string& prefix)" in host
    assert re.search(r"void Learn\(int iters, int episodes, int nniters, int arenaGames, int first_epoch = 0\)", host)
