// AZ.Learn on tic-tac-toe with a replay window whose planes are kept as 2-bit codes (agogo::Config::ReplayPacked,
// agogo_amd/host/agogo.hpp) over the C ABI: az_learn_replay's configuration, arguments and log, followed by a trailing `packed` 0/1 and,
// on every epoch line, the bytes the window holds on the device (agz_replay_storage).  packed = 0 is az_learn_replay's run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../agogo_amd/host/agogo.hpp"

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 2, episodes = argc > 2 ? atoi(argv[2]) : 64, nniters = argc > 3 ? atoi(argv[3]) : 5,
      arenaGames = argc > 4 ? atoi(argv[4]) : 32, budget = argc > 5 ? atoi(argv[5]) : 40;
  const double threshold = argc > 6 ? atof(argv[6]) : 0.52;
  const unsigned long long seed = argc > 7 ? strtoull(argv[7], nullptr, 10) : 1337ull;
  const int spa = argc > 8 ? atoi(argv[8]) : AGZ_INF_NET, spb = argc > 9 ? atoi(argv[9]) : AGZ_INF_NET;
  const int eva = argc > 10 ? atoi(argv[10]) : AGZ_INF_NET, evb = argc > 11 ? atoi(argv[11]) : AGZ_INF_NET;
  const int batch = argc > 12 ? atoi(argv[12]) : 100;
  const long long window = argc > 13 ? atoll(argv[13]) : 600;
  const int steps = argc > 14 ? atoi(argv[14]) : 0;
  const bool symmetric = argc > 15 ? atoi(argv[15]) != 0 : true;
  const bool packed = argc > 16 ? atoi(argv[16]) != 0 : true;
  try {
    agz::Ctx ctx(0);
    agogo::Config conf;
    conf.Name = "Tic Tac Toe";
    conf.NNConf = dual::DefaultConf(3, 3, 10);
    conf.NNConf.BatchSize = batch; conf.NNConf.Features = 2; conf.NNConf.K = 3; conf.NNConf.SharedLayers = 3;
    conf.MCTSConf = mcts::DefaultConfig(3);
    conf.MCTSConf.Budget = budget;
    conf.UpdateThreshold = threshold;
    conf.SelfPlayInferencer[0] = spa; conf.SelfPlayInferencer[1] = spb; conf.EvalInferencer[0] = eva; conf.EvalInferencer[1] = evb;
    conf.ReplayWindow = window; conf.ReplaySteps = steps; conf.ReplaySymmetric = symmetric; conf.ReplayPacked = packed;
    agogo::AZ az(ctx, agogo::GameSpec{AGZ_GAME_MNK, 3, 3, 3, 0.f}, conf, seed);
    az.Learn(iters, episodes, nniters, arenaGames);
    const long long window_bytes = az.window ? (long long)az.window->DeviceBytes() : 0;
    int32_t is_packed = 0;
    if (az.window) agz::check(agz_replay_storage(az.window->h, &is_packed, nullptr, nullptr), "window storage");
    bool ok = (int)az.log.size() == iters && (!az.window || (is_packed != 0) == packed);
    size_t cumulative = 0;
    for (auto& e : az.log) {
      printf("epoch %d examples %zu batches %d cost %.9g A %ld B %ld draw %ld killedA %d a_id %d", e.epoch, e.examples, e.batches, e.cost,
             e.a_wins, e.b_wins, e.draws, (int)e.killedA, e.a_id);
      if (window > 0) printf(" window %zu steps %d window_bytes %lld", e.window, e.steps, window_bytes);
      printf("\n");
      cumulative += e.examples;
      ok = ok && e.batches >= 1 && std::isfinite(e.cost) && e.a_wins + e.b_wins + e.draws == arenaGames;
      if (window > 0) {
        const int want_steps = steps > 0 ? steps : e.batches * nniters;
        ok = ok && e.window == std::min<size_t>((size_t)window, cumulative) && e.steps == want_steps && (int)e.window >= batch;
      } else {
        ok = ok && (int)e.examples >= batch && e.window == 0 && e.steps == 0;
      }
    }
    for (int id : az.stats.Creation) {
      printf("stats net %d:", id);
      for (size_t j = 0; j < az.stats.Wins[id].size(); j++) printf(" %g/%g/%g", az.stats.Wins[id][j], az.stats.Losses[id][j], az.stats.Draws[id][j]);
      printf("\n");
    }
    printf("AZ_LEARN_REPLAY_PACKED %s\n", ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    printf("AZ_LEARN_REPLAY_PACKED EXCEPTION %s\n", e.what());
    return 2;
  }
}
