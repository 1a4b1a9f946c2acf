"""CPU: the arena checkpoint format, checked on the code the arena runs.

agogo_amd/csrc/arena_ckpt.hpp is the only place that knows the bytes of an agz_arena_save file and the only place that validates one.  It
includes nothing from HIP, so tests/cpp/arena_ckpt_check.cpp runs it under g++ on a toy arena (3 games of a 2x3 board, 6 trees with 1, 0,
5, 9, 2, 4 live nodes, two of them in pool 1, a 2-deep ring, 4 example rows chained across two games), written and read in chunks that cut
trees: the round trip, EVERY truncation, a trailing byte, and one corruption per rule scan() enforces.  The bytes themselves are rebuilt
here with `struct` from the format comment of the header, so the comment and the code cannot drift.  The same program holds the header's
chunk planners (node_chunks, example_chunks), by which engine.hip streams the nodes and the examples, to their contract."""
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join("tests", "cpp", "arena_ckpt_check.cpp")
HEADER = os.path.join("agogo_amd", "csrc", "arena_ckpt.hpp")
G, T, P, R, S, CELLS, A, F, E = 3, 6, 8, 2, 10, 6, 6, 2, 4
N_NODES, CUR_POOL = (1, 0, 5, 9, 2, 4), (0, 0, 1, 0, 1, 0)
LINKS = [[(-1, 0)], [], [(1, 4)] + [(-1, 0)] * 4, [(1, 3), (-1, 0), (4, 5)] + [(-1, 0)] * 6, [(1, 1), (-1, 0)], [(1, 2), (3, 1), (-1, 0), (-1, 0)]]


def pad(cells):
    return list(cells) + [0] * (P - CELLS)


def arr(fmt, values):
    values = list(values)
    return struct.pack("<%d%s" % (len(values), fmt), *values)


def expected():
    """the toy arena's file, from the format comment of arena_ckpt.hpp"""
    b = b"AGZARN01"
    b += struct.pack("<4if2i", 0, 2, 3, 2, 0.5, 6, 0)                                  # agz_game_conf (max_moves resolved)
    b += struct.pack("<f4iIfifi", 1.0, 2, 3, 0, 4, 0, 0.0, 1, 0.0, 0)                  # agz_mcts_conf
    b += struct.pack("<5I", G, 1, P, R, S)                                             # n_games, lanes, CELLS_PAD, RING, moves_stride
    b += struct.pack("<3QiI", 0x1111222233334444, 0x5555666677778888, 7, 5, 0)         # seed, seed0, prep_expand_seen, moves_done, restart
    gs = range(G)
    b += arr("b", sum((pad((g + i) % 3 for i in range(CELLS)) for g in gs), []))                                   # board
    b += arr("b", sum((pad((g + r + i) % 3 for i in range(CELLS)) for g in gs for r in range(R)), []))             # ring
    for col in ([1 + g % 2 for g in gs], [g + 2 for g in gs], list(gs), [g % 2 for g in gs], [int(g == 1) for g in gs], [2 if g == 1 else 0 for g in gs],
                [int(g != 2) for g in gs], [g - 1 for g in gs]):                       # to_move, ply, passes, pass_count, ended, winner, a_is_black, last_move
        b += arr("i", col)
    b += arr("f", [0.5 * g for g in gs]) + arr("f", [1.5 * g for g in gs]) + arr("I", [0xABCD0000 + g for g in gs])
    b += arr("h", [(g + j) % A for g in gs for j in range(S)]) + arr("h", [(g + 2 * j) % A - 1 for g in gs for j in range(S)])
    b += arr("i", [g + 3 for g in gs]) + arr("i", [g % 2 for g in gs]) + arr("Q", [0x0102030405060708 * (g + 1) for g in gs])
    b += arr("i", [2, -1, 3]) + arr("i", [g - 2 for g in gs])                          # ex_last, best_out
    ts = range(T)
    pc_n = [t % 4 for t in ts]
    for col in (N_NODES, CUR_POOL, [int(n > 0) for n in N_NODES], [int(t % 2 == 0) for t in ts], [t % 3 for t in ts], [int(t == 3) for t in ts],
                [int(t == 4) for t in ts], pc_n):                                      # n_nodes .. pc_n
        b += arr("i", col)
    b += arr("b", sum((pad((t + 2 * i) % 3 for i in range(CELLS)) for t in ts), []))   # prev_board
    b += arr("Q", [0x1000000000000001 * (t + 1) for t in ts])                          # rng
    for t in ts:                                                                       # the first pc_n[t] cached policies of every tree
        b += arr("I", [0x9000 + 16 * t + q for q in range(pc_n[t])]) + arr("h", [(t + q) % (A + 1) - 1 for q in range(pc_n[t])])
    nodes = [(t, i) for t in ts for i in range(N_NODES[t])]                            # tree by tree, the live prefix
    b += struct.pack("<Q", len(nodes))
    b += arr("f", [0.25 * i + t for t, i in nodes]) + arr("I", [10 * t + i + 1 for t, i in nodes]) + arr("f", [-0.5 * i - t for t, i in nodes])
    b += arr("i", [LINKS[t][i][0] for t, i in nodes]) + arr("h", [LINKS[t][i][1] for t, i in nodes])
    b += arr("h", [-1 if i == 0 else (i + t) % A for t, i in nodes])
    b += arr("Q", [1000 * k + 7 for k in range(16)])                                   # counters
    b += struct.pack("<Q", E)
    b += arr("f", [e + j / 16.0 for e in range(E) for j in range(F * CELLS)]) + arr("f", [(7 * e + j) / 32.0 for e in range(E) for j in range(A + 1)])
    b += arr("f", [1.0, 2.0, -1.0, 1.0]) + arr("i", [0, 2, 0, 2]) + arr("i", [-1, -1, 0, 1]) + arr("B", [1, 0, 1, 0])
    return b + b"AGZARNZZ" + struct.pack("<Q", len(b) + 16)


def run_check(root, tmp_path, extra=()):
    """compile the check against the header under `root`, run it, compare the file it wrote; the first thing that is wrong, or None"""
    exe, out_dir = str(tmp_path / "arena_ckpt_check"), tmp_path / "files"
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(root, CHECK)])
    out = subprocess.run([exe, str(out_dir)], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 or "ARENA CKPT OK" not in out.stdout:
        return "the check failed:\n" + out.stdout[-3000:] + out.stderr[-3000:]
    if open(out_dir / "toy.bin", "rb").read() != expected():
        return "the bytes of the toy file moved"
    return None


def test_the_codec_writes_the_documented_bytes_and_refuses_every_bad_file(tmp_path):
    assert run_check(ROOT, tmp_path) is None


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone program again, instrumented: every truncated and corrupted file walks scan()'s reads, seeks and index checks"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        flags = []                                                                    # this g++ does not link the runtimes: the plain program
    assert run_check(ROOT, tmp_path, extra=flags) is None


def test_a_mutated_header_fails_the_check(tmp_path):
    """the check is not vacuous: two runs swapped, a rule of scan() dropped or weakened, a file that may run on, a planner that breaks its
    contract — each is caught by the program or by the byte comparison"""
    hdr = open(os.path.join(ROOT, HEADER)).read()
    muts = [("constexpr uint64_t NODE_SIZE[NODE_FIELDS] = {4, 4, 4, 4, 2, 2};", "constexpr uint64_t NODE_SIZE[NODE_FIELDS] = {4, 4, 4, 2, 4, 2};"),
            ("if (off <= i || off >= n)", "if (off < 0 || off >= n)"), ("if (ep[i] < -1 || ep[i] >= e)", "if (ep[i] < -1 || ep[i] >= (int64_t)E)"),
            ("if ((uint64_t)len != l.total)", "if ((uint64_t)len < l.total)"), ("f(s.ex_last, 1); f(s.best_out, 1);", "f(s.best_out, 1); f(s.ex_last, 1);"),
            ("if (claimed[(size_t)j]) return", "if (false) return"),
            # the planners: a chunk no longer ends on a tree boundary (its launch outgrows the grid), a run's last chunk runs past its end
            ("    if (f[t1] > n0) n1 = f[t1];", "    ;"), ("out.push_back({k, a, std::min(a + step, l.examples * es[k]), 0, 0});", "out.push_back({k, a, a + step, 0, 0});")]
    os.makedirs(tmp_path / "agogo_amd" / "csrc")
    os.makedirs(tmp_path / "tests" / "cpp")
    shutil.copy(os.path.join(ROOT, CHECK), tmp_path / CHECK)
    for old, new in muts:
        assert hdr.count(old) == 1, old
        (tmp_path / HEADER).write_text(hdr.replace(old, new))
        assert run_check(str(tmp_path), tmp_path) is not None, "mutation %r passes the check" % new
    (tmp_path / HEADER).write_text(hdr)
    assert run_check(str(tmp_path), tmp_path) is None
