// The trainer's checkpoint file (agz_trainer_save / agz_trainer_load): its byte layout, and nothing else.  Host-only: include/agz.h and the
// standard library, so tests/cpp/ckpt_check.cpp checks this very code under g++ (tests/test_ckpt_cpu.py).  train.hip describes a trainer as
// a Layout, hands tensors over through a callback (write) and reads them at the offsets scan() returns; it knows nothing of the bytes.
//
// Every learnable is stored in its full batch-shaped form (AZ.Save / AZ.Load, agogo.go:175-209, for the side that keeps learning).  All
// words are little-endian, nothing is padded.  A file is
//
//     magic words | agz_net_conf (40 bytes) | uint64 n_tensors | group 0 | [options | group 1 [| group 2]] | [BatchNorm block]
//
//     group       per tensor, in the order of agz_trainer_param_info: uint64 n, float32[n]
//     group 0     the learnables
//     options     velocity: agz_solver_conf (16 bytes, momentum != 0)
//                 Adam:     agz_solver_conf (16 bytes, momentum == 0), agz_adam_conf (16 bytes, on == 1), uint64 t (the solver steps taken)
//     group 1     velocity: every tensor's velocity;  Adam: every tensor's first moment
//     group 2     Adam: every tensor's second moment
//     BatchNorm   float32 momentum, uint32 on, uint32 n_ops, then per op (the order of agz_net_set_bn_stats):
//                 uint64 C, double N, double S_mean[C], double S_var[C]
//
// and the magic words name which of the optional parts follow (Form below):
//
//     trainer state                              magic words
//     ----------------------------------------   ----------------------------------------------------------------
//     no solver state                            "AGZTRN01"
//     a velocity (momentum != 0)                 "AGZTRN02"
//     Adam on                                    "AGZTRN04"
//     ... with running BatchNorm statistics      "AGZTRN03", uint32 inner = 1 / 2 / 3 (none / velocity / Adam)
//     a tied trainer, without statistics         "AGZTRN05", uint32 form = 1 / 2 / 4, uint32 flags = 1
//     a tied trainer, with statistics            "AGZTRN05", uint32 form = 3, uint32 flags = 1, uint32 inner = 1 / 2 / 3
//
// flags: bit 0 = tied, the only one defined and always set.  A tied file holds the tied tensor sizes; at BatchSize 1 they coincide with a
// plain trainer's, and the flag alone tells the two kinds apart.  l2reg / clip without a momentum or Adam are not stored: they are the
// caller's configuration, like lr.  The configuration (and the size of every batch-shaped tensor) is the GLOBAL batch's on a sharded
// trainer: its file is the plain trainer's at that batch size.
//
// What a file does to the trainer that loads it (agz_trainer_load applies it only after scan() has accepted ALL of it):
//     learnables       always set
//     no solver state  the trainer's options stay; its velocity or moments and t are zeroed
//     velocity         the file's solver options and velocity; Adam is turned off
//     Adam             the file's solver options, Adam settings, t and moments; Adam is turned on (a velocity is released)
//     BatchNorm block  the file's tracking setting and state;  without one: the state is reset to N = 0, the setting stays
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "agz.h"

namespace agz {
namespace ckpt {

inline bool solver_conf_valid(const agz_solver_conf* c) {
  return std::isfinite(c->momentum) && std::isfinite(c->l2reg) && std::isfinite(c->clip) && c->momentum >= 0.f && c->momentum < 1.f &&
         c->l2reg >= 0.f && c->clip >= 0.f && c->reserved == 0;
}
inline bool adam_conf_valid(const agz_adam_conf* c) {
  return std::isfinite(c->beta1) && std::isfinite(c->beta2) && std::isfinite(c->eps) && c->beta1 >= 0.f && c->beta1 < 1.f && c->beta2 >= 0.f &&
         c->beta2 < 1.f && c->eps > 0.f && (c->on == 0 || c->on == 1);
}
inline bool bn_momentum_valid(float m) { return std::isfinite(m) && m >= 0.f && m < 1.f; }

// ---- which optional parts a file has <-> its magic words ------------------------------------------------------------------------------
enum State { NONE = 0, VELOCITY = 1, ADAM = 2 };
struct Form { bool tied; State state; bool bn; };
inline int groups(State s) { return 1 + (int)s; }   // tensor groups in the file

inline bool write_form(FILE* f, Form m) {
  const uint32_t inner = (uint32_t)m.state + 1, form = m.bn ? 3u : m.state == ADAM ? 4u : inner, flags = 1u;
  char magic[9] = "AGZTRN00";
  magic[7] = (char)('0' + (m.tied ? 5u : form));
  return fwrite(magic, 1, 8, f) == 8 && (!m.tied || (fwrite(&form, 4, 1, f) == 1 && fwrite(&flags, 4, 1, f) == 1)) &&
         (!m.bn || fwrite(&inner, 4, 1, f) == 1);
}
inline bool read_form(FILE* f, Form* m) {
  char magic[8];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "AGZTRN0", 7) != 0 || magic[7] < '1' || magic[7] > '5') return false;
  uint32_t form = (uint32_t)(magic[7] - '0'), flags = 0, inner = 0;
  m->tied = form == 5;
  if (m->tied && (fread(&form, 4, 1, f) != 1 || fread(&flags, 4, 1, f) != 1 || form < 1 || form > 4 || flags != 1u)) return false;
  m->bn = form == 3;
  if (m->bn && (fread(&inner, 4, 1, f) != 1 || inner < 1 || inner > 3)) return false;
  m->state = m->bn ? (State)(inner - 1) : form == 4 ? ADAM : (State)(form - 1);
  return true;
}

// ---- what the trainer says about itself, and what a file says ---------------------------------------------------------------------------
struct Tensor { uint64_t count; bool batch; };   // floats in the FILE (all ranks' rows); batch-shaped = its rows are split over the ranks
struct Layout {
  agz_net_conf conf;              // stored and compared (BatchSize: the global batch)
  bool tied;
  std::vector<Tensor> tensors;
  std::vector<uint64_t> bn_C;     // channels of every BatchNorm op
};
struct Options { agz_solver_conf solver; agz_adam_conf adam; uint64_t step; };   // (solver: VELOCITY and ADAM; adam, step: ADAM)
struct BnBlock { float lam; uint32_t on; std::vector<double> n; std::vector<std::vector<double>> sm, sv; };

// rank's rows of tensor t whose floats start at file offset `off`: {offset, count}.  One rank: the whole tensor.
inline std::pair<long, uint64_t> rows(const Tensor& t, long off, int rank, int n_ranks) {
  if (!t.batch) return {off, t.count};
  const uint64_t n = t.count / (uint64_t)n_ranks;
  return {off + (long)(n * 4 * (uint64_t)rank), n};
}

// ---- writer: header, groups, BatchNorm block.  source(group, index) -> {floats, count} of one tensor; it is called for every tensor of
// every group, in file order, whatever failed before and also when f == nullptr (a rank of a sharded trainer that holds no file: fetching
// a tensor is collective there).  A null pointer or a count that is not the layout's fails the write.
using Source = std::function<std::pair<const float*, uint64_t>(int group, size_t index)>;
inline bool write(FILE* f, const Layout& lay, Form m, const Options& opt, const BnBlock& bn, const Source& source) {
  const uint64_t nt = lay.tensors.size();
  bool ok = f && write_form(f, m) && fwrite(&lay.conf, sizeof(lay.conf), 1, f) == 1 && fwrite(&nt, 8, 1, f) == 1;
  for (int g = 0; g < groups(m.state); g++) {
    if (ok && g == 1) ok = fwrite(&opt.solver, sizeof(opt.solver), 1, f) == 1;
    if (ok && g == 1 && m.state == ADAM) ok = fwrite(&opt.adam, sizeof(opt.adam), 1, f) == 1 && fwrite(&opt.step, 8, 1, f) == 1;
    for (size_t i = 0; i < lay.tensors.size(); i++) {
      const std::pair<const float*, uint64_t> t = source(g, i);
      if (ok) ok = t.first && t.second == lay.tensors[i].count && fwrite(&t.second, 8, 1, f) == 1 && fwrite(t.first, 4, t.second, f) == t.second;
    }
  }
  if (!ok || !m.bn) return ok;
  const uint32_t nops = (uint32_t)lay.bn_C.size();
  ok = bn.n.size() == nops && bn.sm.size() == nops && bn.sv.size() == nops && fwrite(&bn.lam, 4, 1, f) == 1 && fwrite(&bn.on, 4, 1, f) == 1 &&
       fwrite(&nops, 4, 1, f) == 1;
  for (uint32_t i = 0; ok && i < nops; i++) {
    const uint64_t C = lay.bn_C[i];
    ok = bn.sm[i].size() == C && bn.sv[i].size() == C && fwrite(&C, 8, 1, f) == 1 && fwrite(&bn.n[i], 8, 1, f) == 1 &&
         fwrite(bn.sm[i].data(), 8, C, f) == C && fwrite(bn.sv[i].data(), 8, C, f) == C;
  }
  return ok;
}

// ---- scan: the WHOLE file is read and checked against the layout — magic words, configuration, tensor count, every count word, the
// options, the BatchNorm block, and that it ends exactly where the layout says — before the caller changes anything.  The floats
// themselves are skipped, not read.
enum Status {
  OK = 0,
  NOT_THIS,   // no checkpoint, or of another configuration
  KIND,       // a tied trainer's file for a plain trainer or the reverse (form.tied is the file's)
  BROKEN      // truncated, too long, or inconsistent
};
struct Scan {
  Form form;
  Options opt;
  BnBlock bn;
  std::vector<long> off[3];   // [group][tensor]: file offset of the tensor's floats
};

inline bool read_bn(FILE* f, const Layout& lay, BnBlock& b) {
  uint32_t nops = 0;
  if (fread(&b.lam, 4, 1, f) != 1 || fread(&b.on, 4, 1, f) != 1 || fread(&nops, 4, 1, f) != 1) return false;
  if (!bn_momentum_valid(b.lam) || b.on > 1 || nops != lay.bn_C.size()) return false;
  b.n.resize(nops); b.sm.resize(nops); b.sv.resize(nops);
  for (uint32_t i = 0; i < nops; i++) {
    uint64_t C = 0;
    if (fread(&C, 8, 1, f) != 1 || C != lay.bn_C[i] || fread(&b.n[i], 8, 1, f) != 1 || !(std::isfinite(b.n[i]) && b.n[i] > 0)) return false;
    b.sm[i].resize(C); b.sv[i].resize(C);
    if (fread(b.sm[i].data(), 8, C, f) != C || fread(b.sv[i].data(), 8, C, f) != C) return false;
    for (uint64_t c = 0; c < C; c++) if (!std::isfinite(b.sm[i][c]) || !std::isfinite(b.sv[i][c])) return false;
  }
  return true;
}

inline Status scan(FILE* f, const Layout& lay, Scan* out) {
  for (auto& o : out->off) o.clear();
  agz_net_conf c;
  uint64_t nt = 0;
  if (fseek(f, 0, SEEK_END) != 0) return NOT_THIS;
  const long len = ftell(f);
  if (len < 0 || fseek(f, 0, SEEK_SET) != 0 || !read_form(f, &out->form) || fread(&c, sizeof(c), 1, f) != 1 || fread(&nt, 8, 1, f) != 1) return NOT_THIS;
  if (out->form.tied != lay.tied) return KIND;
  if (memcmp(&c, &lay.conf, sizeof(c)) != 0 || nt != lay.tensors.size()) return NOT_THIS;
  Options& o = out->opt;
  bool ok = true;
  for (int g = 0; ok && g < groups(out->form.state); g++) {
    if (g == 1) ok = fread(&o.solver, sizeof(o.solver), 1, f) == 1 && solver_conf_valid(&o.solver) && (o.solver.momentum != 0.f) == (out->form.state == VELOCITY);
    if (ok && g == 1 && out->form.state == ADAM)
      ok = fread(&o.adam, sizeof(o.adam), 1, f) == 1 && fread(&o.step, 8, 1, f) == 1 && adam_conf_valid(&o.adam) && o.adam.on == 1;
    for (size_t i = 0; ok && i < lay.tensors.size(); i++) {
      uint64_t cnt = 0;
      ok = fread(&cnt, 8, 1, f) == 1 && cnt == lay.tensors[i].count;
      out->off[g].push_back(ftell(f));
      ok = ok && out->off[g].back() >= 0 && fseek(f, (long)(cnt * 4), SEEK_CUR) == 0;
    }
  }
  if (ok && out->form.bn) ok = read_bn(f, lay, out->bn);
  if (ok && ftell(f) == len) return OK;   // (a seek beyond the end succeeds: a file cut inside the floats is caught here)
  for (auto& v : out->off) v.clear();
  return BROKEN;
}

}  // namespace ckpt
}  // namespace agz
