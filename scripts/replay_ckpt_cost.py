"""What a replay window checkpoint (agz_replay_save / agz_replay_load) costs at the headline row shape (19x19, 18 planes, policy 362) on one
GPU: wall time and GB/s of a save and of a load of a window of --rows rows (default 131 072) in both forms, and the split of a load between
its validating pass and its committing pass.  One JSON object a line:

  save        agz_replay_save between two clock reads (digest, chunked device-to-host copies under the file writes, fsync, rename)
  load        agz_replay_load into a fresh window of the same capacity and form: both passes.  `cache` says whether the file's pages were
              left in the page cache by the save ("warm") or dropped for this file first with posix_fadvise(DONTNEED) ("cold")
  validate    the same call on a copy of the file whose digest word is wrong: the header passes, the WHOLE validating pass runs (every
              chunk staged, scanned and digested), the call ends with AGZ_E_INVALID and the committing pass never starts.  load - validate
              is the committing pass.
  crossform   a load of the fp32 file into a packed window and of the packed file into an fp32 window (warm)

The window's rows are drawn over agz_encoder_palette(AGZ_ENC_WQ); after every load the digest is compared with the saved window's.  The
files go to --dir (default: the temporary directory), whose file system is named from /proc/mounts, and are removed at the end.
Figures: profiles/replay_ckpt.md."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import agogo_amd as A
from agogo_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=131072)
ap.add_argument("--dir", default=tempfile.gettempdir())
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

S, F = 19, 18
A1, MM = S * S + 1, S * S
ROW = {False: (F * MM + A1 + 1) * 4, True: (F * ((MM + 15) // 16) + A1 + 1) * 4}
INVALID = -1


def file_system(path):
    path, best = os.path.realpath(path), ("", "?", "?")
    for line in open("/proc/mounts"):
        dev, mount, kind = line.split()[:3]
        if (path == mount or path.startswith(mount.rstrip("/") + "/")) and len(mount) > len(best[0]):
            best = (mount, kind, dev)
    return {"mount": best[0], "type": best[1], "device": best[2]}


def drop_pages(path):
    fd = os.open(path, os.O_RDONLY)
    os.fsync(fd)
    os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
    os.close(fd)


ctx = A.Ctx(0)
pal = capi.encoder_palette(capi.ENC_WQ)
rng = np.random.default_rng(0)
print(json.dumps({"rows": args.rows, "dir": args.dir, "file_system": file_system(args.dir), "row_bytes": {"fp32": ROW[False], "packed": ROW[True]}}), flush=True)

windows = {packed: A.Replay(ctx, F, S, S, A1, args.rows, palette=pal if packed else None) for packed in (False, True)}
for a in range(0, args.rows, 8192):                                      # the same rows into both, 8192 at a time
    n = min(8192, args.rows - a)
    x = rng.choice(pal.view(np.uint32), size=(n, F * MM)).astype(np.uint32).view(np.float32)
    pi, v = rng.random((n, A1), np.float32), rng.choice(np.array([-1, 0, 1], np.float32), n).astype(np.float32)
    for rp in windows.values():
        rp.append_host(x, pi, v)
digest = windows[False].digest()
assert windows[True].digest() == digest and len(windows[False]) == args.rows

paths = {}
for packed, rp in windows.items():
    form = "packed" if packed else "fp32"
    path = paths[packed] = os.path.join(args.dir, "replay_ckpt_cost_%s_%d.rpw" % (form, os.getpid()))
    for run in range(args.runs):
        t0 = time.perf_counter()
        rp.save(path)
        dt = time.perf_counter() - t0
        size = os.path.getsize(path)
        print(json.dumps({"part": "save", "form": form, "run": run, "bytes": size, "s": round(dt, 4), "GBps": round(size / dt / 1e9, 3)}), flush=True)
    assert size == 96 + args.rows * ROW[packed]
    bad = path + ".bad"                                                  # the same file with another digest word: validated, then refused
    with open(path, "rb") as f, open(bad, "wb") as g:
        g.write(f.read(72))
        g.write(int((digest + 1) % 2 ** 64).to_bytes(8, "little"))
        f.seek(80)
        while True:
            block = f.read(64 << 20)
            if not block:
                break
            g.write(block)
    for cache in ("warm", "cold"):
        for run in range(args.runs):
            for part, name in (("load", path), ("validate", bad)):
                dst = A.Replay(ctx, F, S, S, A1, args.rows, palette=pal if packed else None)
                if cache == "cold":
                    drop_pages(name)
                else:
                    open(name, "rb").read(1)
                t0 = time.perf_counter()
                rc = capi.lib().agz_replay_load(dst.h, os.fsencode(name))
                dt = time.perf_counter() - t0
                if part == "load":
                    assert rc == 0 and dst.digest() == digest and len(dst) == args.rows
                else:
                    assert rc == INVALID and b"digest" in capi.lib().agz_last_error() and len(dst) == 0
                print(json.dumps({"part": part, "form": form, "cache": cache, "run": run, "bytes": size, "s": round(dt, 4),
                                  "GBps": round(size / dt / 1e9, 3)}), flush=True)
                dst.close()
    os.remove(bad)

for packed in (False, True):                                             # the file's form; the window has the other one
    for run in range(args.runs):
        dst = A.Replay(ctx, F, S, S, A1, args.rows, palette=None if packed else pal)
        t0 = time.perf_counter()
        dst.load(paths[packed])
        dt = time.perf_counter() - t0
        assert dst.digest() == digest
        size = os.path.getsize(paths[packed])
        print(json.dumps({"part": "crossform", "file": "packed" if packed else "fp32", "window": "fp32" if packed else "packed", "run": run,
                          "bytes": size, "s": round(dt, 4), "GBps": round(size / dt / 1e9, 3)}), flush=True)
        dst.close()
for path in paths.values():
    os.remove(path)
for rp in windows.values():
    rp.close()
ctx.close()
