// AZ.Learn resumed at an epoch boundary (agogo::AZ::SaveRun / LoadRun / Learn(..., first_epoch), agogo_amd/host/agogo.hpp) on tic-tac-toe
// with a replay window, over the C ABI.  Usage: az_learn_resume MODE PACKED PREFIX [inferencer kind of self-play A, B, evaluation A, B [BatchSize]]
//   MODE full      Learn(3, ...) on one AZ
//   MODE resume    Learn(2, ...), SaveRun(PREFIX); the AZ is destroyed; a newly constructed AZ does LoadRun(PREFIX) and
//                  Learn(1, ..., first_epoch = 2).  Before that, an AZ of another configuration (Budget + 1) and a ".run" file cut by one
//                  byte must each be refused with NOTHING loaded, and so must a set whose ".A" file is not the one the ".run" file was
//                  written beside ("REFUSED" lines).
// Both print the same text if the continuation is the uninterrupted run: one line an epoch with the cost as its bit pattern, the
// statistics, the digest of the final window and a digest of every parameter of A.  Ends with "AZ_LEARN_RESUME OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../agogo_amd/host/agogo.hpp"

static const int EPISODES = 32, NNITERS = 2, GAMES = 8;

static agogo::Config config(bool packed, int budget, const int inf[4], int batch) {
  agogo::Config conf;
  conf.Name = "Tic Tac Toe";
  conf.NNConf = dual::DefaultConf(3, 3, 10);
  conf.NNConf.BatchSize = batch; conf.NNConf.Features = 2; conf.NNConf.K = 3; conf.NNConf.SharedLayers = 3;
  conf.MCTSConf = mcts::DefaultConfig(3);
  conf.MCTSConf.Budget = budget;
  conf.UpdateThreshold = 0.52;
  conf.SelfPlayInferencer[0] = inf[0]; conf.SelfPlayInferencer[1] = inf[1]; conf.EvalInferencer[0] = inf[2]; conf.EvalInferencer[1] = inf[3];
  conf.ReplayWindow = 200; conf.ReplaySteps = 0; conf.ReplaySymmetric = true; conf.ReplayPacked = packed;
  return conf;
}

// FNV-1a over the bytes of every learnable of a trainer, in order
static uint64_t params_digest(const dual::Trainable& t) {
  uint64_t d = 0xcbf29ce484222325ull;
  const int n = agz_trainer_num_params(t.h);
  for (int i = 0; i < n; i++) {
    char name[64];
    size_t len = 0;
    agz::check(agz_trainer_param_info(t.h, i, name, sizeof(name), &len), "param info");
    std::vector<float> v(len);
    agz::check(agz_trainer_get_param(t.h, i, v.data(), len), "get param");
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t k = 0; k < len * 4; k++) d = (d ^ p[k]) * 0x100000001b3ull;
  }
  return d;
}

static void report(agogo::AZ& az) {
  for (auto& e : az.log) {
    uint32_t bits;
    memcpy(&bits, &e.cost, 4);
    printf("epoch %d examples %zu batches %d cost_bits %08x A %ld B %ld draw %ld killedA %d a_id %d window %zu steps %d\n", e.epoch, e.examples,
           e.batches, bits, e.a_wins, e.b_wins, e.draws, (int)e.killedA, e.a_id, e.window, e.steps);
  }
  for (int id : az.stats.Creation) {
    printf("stats net %d:", id);
    for (size_t j = 0; j < az.stats.Wins[id].size(); j++) printf(" %g/%g/%g", az.stats.Wins[id][j], az.stats.Losses[id][j], az.stats.Draws[id][j]);
    printf("\n");
  }
  printf("ids %d %d %d epochs_done %d useDummy %d\n", az.a_id, az.b_id, az.next_id, az.epochs_done, (int)az.useDummy);
  printf("window_digest %016llx\n", (unsigned long long)az.window->Digest());
  printf("a_params_digest %016llx\n", (unsigned long long)params_digest(*az.A));
}

// LoadRun must throw, naming `token`, and leave `az` as it was constructed
static bool refused(agogo::AZ& az, const std::string& prefix, const char* token) {
  const uint64_t before = params_digest(*az.A);
  try {
    az.LoadRun(prefix);
  } catch (const agz::Error& e) {
    const bool untouched = az.epochs_done == 0 && az.log.empty() && az.window->size() == 0 && params_digest(*az.A) == before;
    const bool named = strstr(e.what(), token) != nullptr;
    printf("REFUSED (%s, %s): %s\n", named ? "named" : "NOT NAMED", untouched ? "nothing loaded" : "SOMETHING LOADED", e.what());
    return untouched && named;
  }
  printf("REFUSED: no, LoadRun accepted it\n");
  return false;
}

int main(int argc, char** argv) {
  if (argc < 4) { printf("usage: az_learn_resume full|resume PACKED PREFIX [spa spb eva evb [batch]]\n"); return 2; }
  const std::string mode = argv[1], prefix = argv[3];
  const bool packed = atoi(argv[2]) != 0;
  int inf[4];
  for (int i = 0; i < 4; i++) inf[i] = argc > 4 + i ? atoi(argv[4 + i]) : AGZ_INF_NET;
  const agogo::GameSpec ttt{AGZ_GAME_MNK, 3, 3, 3, 0.f};
  const int budget = 20, batch = argc > 8 ? atoi(argv[8]) : 8;
  try {
    agz::Ctx ctx(0);
    bool ok = true;
    std::unique_ptr<agogo::AZ> az(new agogo::AZ(ctx, ttt, config(packed, budget, inf, batch), 1337));
    if (mode == "full") {
      az->Learn(3, EPISODES, NNITERS, GAMES);
    } else {
      az->Learn(2, EPISODES, NNITERS, GAMES);
      az->SaveRun(prefix);
      az.reset();
      {  // another configuration: refused before A or the window is read
        agogo::AZ other(ctx, ttt, config(packed, budget + 1, inf, batch), 1337);
        ok = refused(other, prefix, "MCTSConf.Budget") && ok;
      }
      {  // a ".run" file cut by one byte
        std::string bytes;
        FILE* f = fopen((prefix + ".run").c_str(), "rb");
        char buf[4096];
        for (size_t n; f && (n = fread(buf, 1, sizeof(buf), f)) > 0;) bytes.append(buf, n);
        if (f) fclose(f);
        for (const char* ext : {".A", ".window"}) {   // the other two files under the cut run's name, so that only the ".run" is wrong
          FILE* in = fopen((prefix + ext).c_str(), "rb");
          FILE* out = fopen((prefix + "_cut" + ext).c_str(), "wb");
          for (size_t n; in && out && (n = fread(buf, 1, sizeof(buf), in)) > 0;) ok = fwrite(buf, 1, n, out) == n && ok;
          ok = in && out && ok;
          if (in) fclose(in);
          if (out) fclose(out);
        }
        FILE* g = fopen((prefix + "_cut.run").c_str(), "wb");
        ok = g && bytes.size() > 1 && fwrite(bytes.data(), 1, bytes.size() - 1, g) == bytes.size() - 1 && ok;
        if (g) fclose(g);
        agogo::AZ same(ctx, ttt, config(packed, budget, inf, batch), 1337);
        ok = refused(same, prefix + "_cut", "malformed") && ok;
        // the whole ".run" beside a ".A" that differs in its last byte, as after a SaveRun that did not finish
        FILE* r = fopen((prefix + "_cut.run").c_str(), "wb");
        ok = r && fwrite(bytes.data(), 1, bytes.size(), r) == bytes.size() && ok;
        if (r) fclose(r);
        FILE* a = fopen((prefix + "_cut.A").c_str(), "r+b");
        int last = EOF;
        ok = a && fseek(a, -1, SEEK_END) == 0 && (last = fgetc(a)) != EOF && fseek(a, -1, SEEK_END) == 0 && fputc(last ^ 1, a) != EOF && ok;
        if (a) fclose(a);
        ok = refused(same, prefix + "_cut", "is not the trainer file") && ok;
      }
      az.reset(new agogo::AZ(ctx, ttt, config(packed, budget, inf, batch), 1337));
      az->LoadRun(prefix);
      ok = az->epochs_done == 2 && az->log.size() == 2 && ok;
      az->Learn(1, EPISODES, NNITERS, GAMES, az->epochs_done);
    }
    ok = az->log.size() == 3 && az->epochs_done == 3 && ok;
    int32_t is_packed = 0;
    agz::check(agz_replay_storage(az->window->h, &is_packed, nullptr, nullptr), "window storage");
    ok = (is_packed != 0) == packed && ok;
    report(*az);
    printf("AZ_LEARN_RESUME %s\n", ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    printf("AZ_LEARN_RESUME EXCEPTION %s\n", e.what());
    return 2;
  }
}
