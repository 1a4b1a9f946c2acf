// A file that replaces `path` whole or not at all (agz_arena_save, agz_replay_save).  Host-only, the standard library and POSIX: the bytes
// go to path + ".tmp"; commit() makes them durable and renames the temporary file over `path`; a file that is not committed — a failed
// write, a failed commit, an early return — is closed and removed, and `path` keeps what it held.  The callers word the errors.
#pragma once
#include <cstdio>
#include <string>
#include <unistd.h>

namespace agz {

struct AtomicFile {
  enum End { DONE, WRITE_FAILED, RENAME_FAILED };
  const std::string path, tmp;
  FILE* f;   // nullptr: the temporary file could not be opened (nothing was touched)
  explicit AtomicFile(const char* p) : path(p), tmp(path + ".tmp"), f(fopen(tmp.c_str(), "wb")) {}
  AtomicFile(const AtomicFile&) = delete;
  End commit() {
    const bool flushed = fflush(f) == 0 && fsync(fileno(f)) == 0;
    const bool closed = fclose(f) == 0;
    f = nullptr;
    const End e = !(flushed && closed) ? WRITE_FAILED : rename(tmp.c_str(), path.c_str()) != 0 ? RENAME_FAILED : DONE;
    if (e != DONE) remove(tmp.c_str());
    return e;
  }
  ~AtomicFile() { if (f) { fclose(f); remove(tmp.c_str()); } }
};

}  // namespace agz
