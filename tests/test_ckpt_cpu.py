"""CPU: the trainer's checkpoint format, checked on the code the trainer runs.

agogo_amd/csrc/ckpt.hpp is the only place that knows the bytes of an agz_trainer_save file: the magic words of the twelve forms, the
writer, and scan(), which validates a whole file before agz_trainer_load changes anything.  It includes nothing from HIP, so
tests/cpp/ckpt_check.cpp runs it under g++ on a toy layout (5 tensors of 1, 2, 3, 7, 4 floats, the second and fourth batch-shaped; 3
BatchNorm ops of 3, 2, 1 channels): round trips, three ranks' rows, EVERY truncation of every form, and every inconsistent file of the
right length.  The bytes themselves are compared here with bytes built by `struct` from the format as it was documented before the codec
existed: the format did not move."""
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join("tests", "cpp", "ckpt_check.cpp")
HEADER = os.path.join("agogo_amd", "csrc", "ckpt.hpp")
COUNT, BN_C = (1, 2, 3, 7, 4), (3, 2, 1)
FORMS = [(tied, state, bn) for tied in (False, True) for state in (0, 1, 2) for bn in (False, True)]   # state: none, velocity, Adam


def expected(tied, state, bn):
    """the file of the toy layout, from the format comment that stood above agz_trainer_save"""
    conf = struct.pack("<9if", 3, 1, 8, 2, 3, 3, 2, 10, 0, 0.5)                      # agz_net_conf
    def group(g):
        return b"".join(struct.pack("<Q%df" % n, n, *[1000.0 * g + 100.0 * i + e + 0.5 for e in range(n)]) for i, n in enumerate(COUNT))
    body = conf + struct.pack("<Q", len(COUNT)) + group(0)                            # the 01 payload
    if state == 1:                                                                    # 02: agz_solver_conf, every tensor's velocity
        body += struct.pack("<3fi", 0.5, 0.25, 2.0, 0) + group(1)
    if state == 2:                                                                    # 04: solver (momentum 0), agz_adam_conf, uint64 t, m, v
        body += struct.pack("<3fi", 0.0, 0.25, 2.0, 0) + struct.pack("<3fi", 0.75, 0.875, 0.0078125, 1) + struct.pack("<Q", 0x0102030405)
        body += group(1) + group(2)
    form = (1, 2, 4)[state]
    if bn:                                                                            # 03: uint32 inner form, that body, the BatchNorm block
        body = struct.pack("<I", state + 1) + body + struct.pack("<fII", 0.75, 1, len(BN_C))
        for i, C in enumerate(BN_C):
            body += struct.pack("<Qd", C, 2.5 + i) + struct.pack("<%dd" % C, *[10.0 * i + c + 0.25 for c in range(C)])
            body += struct.pack("<%dd" % C, *[100.0 + 10.0 * i + c + 0.125 for c in range(C)])
        form = 3
    if tied:                                                                          # 05: uint32 inner form, uint32 flags = 1, that file after its magic
        return b"AGZTRN05" + struct.pack("<II", form, 1) + body
    return b"AGZTRN0%d" % form + body


def run_check(root, tmp_path, extra=()):
    """compile the check against the header under `root`, run it, compare the twelve files it wrote; the first thing that is wrong, or None"""
    exe, out_dir = str(tmp_path / "ckpt_check"), tmp_path / "files"
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(root, CHECK)])
    out = subprocess.run([exe, str(out_dir)], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 or "CKPT OK" not in out.stdout:
        return "the check failed:\n" + out.stdout[-3000:] + out.stderr[-3000:]
    for tied, state, bn in FORMS:
        got = open(out_dir / ("form_%s%d%s.bin" % ("pt"[tied], state, "nb"[bn])), "rb").read()
        if got != expected(tied, state, bn):
            return "the bytes of form (tied %d, state %d, bn %d) moved" % (tied, state, bn)
    return None


def test_the_codec_writes_the_documented_bytes_and_refuses_every_bad_file(tmp_path):
    assert run_check(ROOT, tmp_path) is None


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone program again, instrumented: every truncated file walks scan()'s reads and seeks at the edge of the data"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        flags = []                                                                    # this g++ does not link the runtimes: the plain program
    assert run_check(ROOT, tmp_path, extra=flags) is None


def test_a_mutated_header_fails_the_check(tmp_path):
    """the check is not vacuous: the moment groups swapped, a magic digit, the flags word, a file that may run on, count words that go
    unread, a solver block that goes unvalidated — each is caught by the program or by the byte comparison"""
    hdr = open(os.path.join(ROOT, HEADER)).read()
    muts = [("t = source(g, i);", "t = source(g == 0 ? 0 : groups(m.state) - g, i);"), ("(m.tied ? 5u : form)", "(m.tied ? 5u : form + 1)"),
            ("flags = 1u;", "flags = 3u;"), ("ftell(f) == len", "ftell(f) <= len"), ("cnt == lay.tensors[i].count;", "cnt > 0;"),
            ("&& solver_conf_valid(&o.solver) &&", "&&")]
    os.makedirs(tmp_path / "agogo_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "cpp")
    shutil.copy(os.path.join(ROOT, CHECK), tmp_path / CHECK)
    for old, new in muts:
        assert hdr.count(old) == 1, old
        (tmp_path / HEADER).write_text(hdr.replace(old, new))
        assert run_check(str(tmp_path), tmp_path) is not None, "mutation %r passes the check" % new
    (tmp_path / HEADER).write_text(hdr)
    assert run_check(str(tmp_path), tmp_path) is None
