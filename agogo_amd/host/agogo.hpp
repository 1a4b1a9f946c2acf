// Header-only C++ mirror of the reference's operator interface for the hot path, over the C ABI (include/agz.h).
// Same names, argument meaning and error behaviour as the Go types, so host code and tests read like the
// reference's: dual::Config / dual::Dual / dual::Inferencer (dualnet/config.go, dual.go, meta.go),
// mcts::Config (mcts/tree.go:15-29), agogo::Arena (arena.go) for a batch of games.
// Errors: the reference returns `error` or panics; here agz::Error is thrown with agz_last_error().
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/agz.h"

namespace agz {
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int rc, const char* what) {
  if (rc != AGZ_OK) throw Error(std::string(what) + ": " + agz_last_error());
}
struct Ctx {
  agz_ctx* h = nullptr;
  explicit Ctx(int device = 0) { check(agz_ctx_create(device, &h), "agz_ctx_create"); }
  ~Ctx() { agz_ctx_destroy(h); }
  Ctx(const Ctx&) = delete;
  Ctx& operator=(const Ctx&) = delete;
};
}  // namespace agz

namespace dual {
// dualnet/config.go:4-16
struct Config {
  int K = 0, SharedLayers = 0, FC = 0;
  double L2 = 0;
  int BatchSize = 0, Width = 0, Height = 0, Features = 0, ActionSpace = 0;
  bool FwdOnly = false;
  bool IsValid() const { return K >= 1 && ActionSpace >= 3 && SharedLayers >= 0 && FC > 1 && BatchSize >= 1 && Features > 0; }
};
inline int round(int a) {  // config.go:44-58
  int n = a - 1;
  n |= n >> 1; n |= n >> 2; n |= n >> 4; n |= n >> 8; n |= n >> 16; n++;
  int lt = n / 2;
  return (a - lt) < (n - a) ? lt : n;
}
inline Config DefaultConf(int m, int n, int actionSpace) {  // config.go:18-31
  Config c; int k = round((m * n) / 3);
  c.K = k; c.SharedLayers = m; c.FC = 2 * k; c.BatchSize = 256; c.Width = n; c.Height = m; c.Features = 18; c.ActionSpace = actionSpace;
  return c;
}
// dual.Dual (dualnet/dual.go:16-47): parameters live on the device
struct Dual {
  Config conf;
  agz_net* h = nullptr;
  Dual(agz::Ctx& ctx, const Config& c, int bn_mode = AGZ_BN_DEGENERATE_EPS) : conf(c) {
    if (!c.IsValid()) throw agz::Error("NNConf is not valid. Unable to proceed");  // agogo.go:42-44 panics
    agz_net_conf nc{c.K, c.SharedLayers, c.FC, c.BatchSize, c.Width, c.Height, c.Features, c.ActionSpace, bn_mode, 1e-5f};
    agz::check(agz_net_create(ctx.h, &nc, &h), "dual.New");
  }
  ~Dual() { agz_net_destroy(h); }
  void Init(uint64_t seed) { agz::check(agz_net_init_random(h, seed), "Dual.Init"); agz::check(agz_net_commit(h), "Dual.Init"); }
  int NumLearnables() const { return agz_net_num_params(h); }  // len(Model())
  void Let(int i, const std::vector<float>& v) { agz::check(agz_net_set_param(h, i, v.data(), v.size()), "G.Let"); }
  void Commit() { agz::check(agz_net_commit(h), "commit"); }
};
// dual.Inferencer (dualnet/meta.go:106-194), batched
struct Inferencer {
  Dual& d;
  explicit Inferencer(Dual& dd) : d(dd) {}
  // Infer: planes [B,F,H,W] -> policy [B,ActionSpace], value [B]
  void Infer(const std::vector<float>& planes, int B, std::vector<float>* policy, std::vector<float>* value) {
    policy->resize((size_t)B * d.conf.ActionSpace);
    value->resize(B);
    agz::check(agz_net_infer(d.h, planes.data(), B, policy->data(), value->data()), "Inferencer.Infer");
  }
};
// The trainable side of dual.Dual: learnables in their FULL (batch-shaped) form + dual.Train (dualnet/meta.go:16-54)
struct Trainable {
  Config conf;
  agz_trainer* h = nullptr;
  Trainable(agz::Ctx& ctx, const Config& c) : conf(c) {
    if (!c.IsValid()) throw agz::Error("NNConf is not valid. Unable to proceed");
    agz_net_conf nc{c.K, c.SharedLayers, c.FC, c.BatchSize, c.Width, c.Height, c.Features, c.ActionSpace, AGZ_BN_DEGENERATE_EPS, 1e-5f};
    agz::check(agz_trainer_create(ctx.h, &nc, &h), "dual.New");
  }
  ~Trainable() { agz_trainer_destroy(h); }
  Trainable(const Trainable&) = delete;
  Trainable& operator=(const Trainable&) = delete;
  void Init(uint64_t seed) { agz::check(agz_trainer_init_random(h, seed), "Dual.Init"); }
  void SetComputeMode(int mode) { agz::check(agz_trainer_set_compute_mode(h, mode), "compute mode"); }  // AGZ_COMPUTE_BF16X3: faster fwd/dgrad
  // the options of the solver dual.Train constructs (meta.go:20: NewVanillaSolver -> WithL2Reg / WithClip / NewMomentum); all 0 = vanilla
  void SetSolver(float momentum, float l2reg = 0.f, float clip = 0.f) {
    agz_solver_conf sc{momentum, l2reg, clip, 0};
    agz::check(agz_trainer_set_solver(h, &sc), "solver options");
  }
  agz_solver_conf Solver() const { agz_solver_conf sc{}; agz::check(agz_trainer_get_solver(h, &sc), "solver options"); return sc; }
  void ResetSolver() { agz::check(agz_trainer_reset_solver(h), "solver reset"); }   // velocity := 0
  // the loss kind (agz_trainer_set_loss): AGZ_LOSS_REFERENCE (default, dual.go:113-121) or AGZ_LOSS_ALPHAZERO (softmax cross-entropy and
  // an MSE on tanh: what the exported network plays).  Configuration like the solver's: no checkpoint stores it.
  void SetLoss(int kind) { agz::check(agz_trainer_set_loss(h, kind), "loss kind"); }
  int Loss() const { int k = 0; agz::check(agz_trainer_get_loss(h, &k), "loss kind"); return k; }
  // running BatchNorm statistics (the reference asks gorgonia for momentum 0.997, ermahagerdmonards.go:54): from here on every training
  // forward feeds the estimates that SwitchToInference, Eval and Save use.  Off by default.
  void TrackBatchNorm(float momentum = 0.997f) { agz::check(agz_trainer_set_bn_tracking(h, 1, momentum), "BatchNorm tracking"); }
  // a held-out loss: the forward pass alone under the tracked statistics; planes [B,F,H,W], pi [B,ActionSpace], v [B]
  float Eval(const std::vector<float>& planes, const std::vector<float>& pi, const std::vector<float>& v) {
    float cost = 0;
    agz::check(agz_trainer_eval(h, planes.data(), pi.data(), v.data(), &cost), "Eval");
    return cost;
  }
  // dual.Infer (meta.go:125-162): copy row 0 of every learnable into an inference net.  After TrackBatchNorm the tracked statistics go
  // with them: a Dual made with AGZ_BN_RUNNING then plays with the statistics the network was trained under.
  void SwitchToInference(Dual& inf) const { agz::check(agz_trainer_export(h, inf.h), "SwitchToInference"); }
  // AZ.Save / AZ.Load (agogo.go:175-209) of the learning side, full batch-shaped learnables
  void Save(const std::string& path) const { agz::check(agz_trainer_save(h, path.c_str()), "AZ.Save"); }
  void Load(const std::string& path) { agz::check(agz_trainer_load(h, path.c_str()), "AZ.Load"); }
};
// dual.Train(d, Xs, policies, values, batches, iterations) — shuffles the three arrays in place like the reference
inline float Train(Trainable& d, std::vector<float>& Xs, std::vector<float>& policies, std::vector<float>& values, int batches,
                   int iterations, uint64_t seed) {
  float cost = 0;
  agz::check(agz_train(d.h, Xs.data(), policies.data(), values.data(), batches, iterations, seed, &cost), "dual.Train");
  return cost;
}
// the same over device tensors (agz_examples_tensors_dev): nothing leaves HBM
inline float TrainDev(Trainable& d, const float* Xs_dev, const float* policies_dev, const float* values_dev, int batches, int iterations,
                      uint64_t seed) {
  float cost = 0;
  agz::check(agz_train_dev(d.h, Xs_dev, policies_dev, values_dev, batches, iterations, seed, &cost), "dual.Train");
  return cost;
}
// build extension: dual.Train's loop over `steps` minibatches sampled from a replay window (agogo::Replay), on the device
inline float TrainReplay(Trainable& d, agz_replay* window, int steps, uint64_t seed, bool symmetric) {
  float cost = 0;
  agz::check(agz_train_replay(d.h, window, steps, seed, symmetric ? 1 : 0, &cost), "dual.Train");
  return cost;
}
// the same on a sharded Trainable, collective: every rank calls it with its own replica of the window and the same arguments; step s trains
// on minibatch s of n_ranks * BatchSize rows.  The replicas' counts — with verify their digests too — are compared at entry.
inline float TrainReplaySharded(Trainable& d, agz_replay* window, int steps, uint64_t seed, bool symmetric, bool verify) {
  float cost = 0;
  agz::check(agz_train_replay_sharded(d.h, window, steps, seed, symmetric ? 1 : 0, verify ? 1 : 0, &cost), "dual.Train");
  return cost;
}
}  // namespace dual

namespace mcts {
enum PassPreference { DontPreferPass = AGZ_DONT_PREFER_PASS, PreferPass = AGZ_PREFER_PASS, DontResign = AGZ_DONT_RESIGN };
// mcts/tree.go:15-29 (Timeout -> exactly Budget simulations)
struct Config {
  float PUCT = 1.0f;
  int M = 0, N = 0, RandomCount = 0;
  int32_t Budget = 10000;
  uint32_t RandomMinVisits = 0;
  float RandomTemperature = 0;
  bool DumbPass = true;
  float ResignPercentage = 0;
  int PassPreference = DontPreferPass;
  bool IsValid() const { return PUCT > 0 && PUCT <= 1; }
};
inline Config DefaultConfig(int boardSize) { Config c; c.M = c.N = boardSize; return c; }  // tree.go:31-41
}  // namespace mcts

namespace agogo {
struct Example { std::vector<float> Board, Policy; float Value; };  // datatypes.go:41-46
// n_games x Arena (arena.go:20-179)
struct Arena {
  agz_arena* h = nullptr;
  int cells, F, A;
  Arena(agz::Ctx& ctx, int kind, int m, int n, int k, float komi, int encoder, const mcts::Config& mc, int n_games, uint64_t seed)
      : cells(m * n), F(encoder == AGZ_ENC_WQ ? 18 : 2), A(kind == AGZ_GAME_C4 ? n : m * n) {
    if (!mc.IsValid()) throw agz::Error("MCTSConf is not valid. Unable to proceed");  // agogo.go:45-47
    agz_game_conf g{kind, m, n, k, komi, 0, encoder};
    agz_mcts_conf c{mc.PUCT, mc.M, mc.N, mc.RandomCount, mc.Budget, mc.RandomMinVisits, mc.RandomTemperature, mc.DumbPass ? 1 : 0,
                    mc.ResignPercentage, mc.PassPreference};
    agz::check(agz_arena_create(ctx.h, &g, &c, n_games, seed, 0, &h), "MakeArena");
  }
  ~Arena() { agz_arena_destroy(h); }
  void SetAgents(dual::Dual* a, dual::Dual* b) {  // nil -> dummyInferer (agogo.go:83-87)
    agz::check(agz_arena_set_inferencer(h, 0, a ? AGZ_INF_NET : AGZ_INF_DUMMY, a ? a->h : nullptr), "Agent A");
    agz::check(agz_arena_set_inferencer(h, 1, b ? AGZ_INF_NET : AGZ_INF_DUMMY, b ? b->h : nullptr), "Agent B");
  }
  // test hook: a synthetic inferencer kind per agent (AGZ_INF_NET keeps the network)
  void SetAgentKinds(int ka, dual::Dual* a, int kb, dual::Dual* b) {
    agz::check(agz_arena_set_inferencer(h, 0, ka, ka == AGZ_INF_NET ? a->h : nullptr), "Agent A");
    agz::check(agz_arena_set_inferencer(h, 1, kb, kb == AGZ_INF_NET ? b->h : nullptr), "Agent B");
  }
  // Tournament use (Agent.Search against an outside opponent, agent.go:76-81): Search() decides and plays one move for
  // every unfinished game; Opponent() applies the outside player's replies (State.Check'ed on the device).
  void Search(int budget) {
    agz::check(agz_arena_begin_move(h), "Agent.Search");
    agz::check(agz_arena_simulate(h, budget), "Agent.Search");
    agz::check(agz_arena_end_move(h, 0), "Agent.Search");
  }
  void SetParallel(int lanes) { agz::check(agz_arena_set_parallel(h, lanes), "SetParallel"); }  // lane-ordered tree-parallel rounds
  // build extension: leaves of network agents evaluated under a board symmetry — AGZ_SYM_OFF (default), AGZ_SYM_RANDOM (one of the eight
  // per position, a function of board, mover and seed) or AGZ_SYM_FIXED + k.  Square boards, not c4.  Not in a checkpoint: set it again.
  void SetLeafSymmetry(int mode, uint64_t seed = 0) { agz::check(agz_arena_set_leaf_symmetry(h, mode, seed), "SetLeafSymmetry"); }
  // build extension: Dirichlet noise on the root priors of every search, P = (1 - eps) p + eps eta, eta ~ Dir(alpha) (agz_arena_set_root_noise);
  // default off.  Not in a checkpoint: set it again after Load.
  void SetRootNoise(float eps = 0.25f, float alpha = 0.3f, bool on = true) {
    const agz_noise_conf conf = {eps, alpha, on ? 1 : 0, 0};
    agz::check(agz_arena_set_root_noise(h, &conf), "SetRootNoise");
  }
  // build extension: the policy row of a recorded example (agz_arena_set_policy_target): AGZ_TARGET_REFERENCE (default) or AGZ_TARGET_VISITS,
  // the root's visit distribution N(a)^(1/temperature) on every searched ply.  Not in a checkpoint: set it again after Load.
  void SetPolicyTarget(int kind, float temperature = 1.f) {
    const agz_target_conf conf = {kind, temperature, {0, 0}};
    agz::check(agz_arena_set_policy_target(h, &conf), "SetPolicyTarget");
  }
  // build extension: playout cap randomization (agz_arena_set_playout_cap): every ply of every game is a full search (Budget simulations,
  // root noise, a recorded row) with probability p_full, else a fast one (fast_budget simulations, no noise, no row); default off.  Not in a
  // checkpoint: set it again after Load.
  void SetPlayoutCap(float p_full, int fast_budget, uint64_t seed = 0, bool on = true) {
    const agz_playout_cap_conf conf = {p_full, fast_budget, on ? 1 : 0, 0, seed};
    agz::check(agz_arena_set_playout_cap(h, &conf), "SetPlayoutCap");
  }
  // build extension: forced playouts at the root with coefficient k and, with prune and AGZ_TARGET_VISITS, the pruned policy target
  // (agz_arena_set_forced_playouts); default off.  Not in a checkpoint: set it again after Load.
  void SetForcedPlayouts(float k, bool prune = true, bool on = true) {
    const agz_forced_conf conf = {k, on ? 1 : 0, prune ? 1 : 0, 0};
    agz::check(agz_arena_set_forced_playouts(h, &conf), "SetForcedPlayouts");
  }
  void Opponent(const std::vector<int32_t>& moves) { agz::check(agz_arena_apply_moves(h, moves.data()), "opponent move"); }
  // Checkpoint of the running arena between two moves, and the continuation from one (agz_arena_save / agz_arena_load): games, trees, RNG
  // states, counters, examples.  The agents, the lanes and the pool policy are not in the file: set them again as they were.
  void Save(const std::string& path) { agz::check(agz_arena_save(h, path.c_str()), "Arena.Save"); }
  void Load(const std::string& path) { agz::check(agz_arena_load(h, path.c_str()), "Arena.Load"); }
  // Play every game to the end, leaving the recorded examples on the device (see Examples::Append)
  void PlayOnDevice(bool record) {
    agz::check(agz_arena_reset(h, nullptr), "Arena.Play");
    agz::check(agz_arena_play(h, 0, record ? 1 : 0), "Arena.Play");
  }
  // Play every game to the end (Arena.Play, arena.go:80-179), recording examples
  std::vector<Example> Play(bool record) {
    agz::check(agz_arena_reset(h, nullptr), "Arena.Play");
    agz::check(agz_arena_play(h, 0, record ? 1 : 0), "Arena.Play");
    int n = 0;
    agz::check(agz_arena_get_examples(h, nullptr, nullptr, nullptr, nullptr, 0, &n), "examples");
    std::vector<float> P((size_t)n * F * cells), Q((size_t)n * (A + 1)), V(n);
    if (n) agz::check(agz_arena_get_examples(h, P.data(), Q.data(), V.data(), nullptr, n, &n), "examples");
    std::vector<Example> ex(n);
    for (int i = 0; i < n; i++) {
      ex[i].Board.assign(P.begin() + (size_t)i * F * cells, P.begin() + (size_t)(i + 1) * F * cells);
      ex[i].Policy.assign(Q.begin() + (size_t)i * (A + 1), Q.begin() + (size_t)(i + 1) * (A + 1));
      ex[i].Value = V[i];
    }
    return ex;
  }
};
// []Example kept on the device (include/agz.h "example sets"): Augmenter, shuffleExamples, prepareExamples
struct Examples {
  agz_examples* h = nullptr;
  Examples(agz::Ctx& ctx, int F, int H, int W, int policyLen) { agz::check(agz_examples_create(ctx.h, F, H, W, policyLen, &h), "Examples"); }
  ~Examples() { agz_examples_destroy(h); }
  Examples(const Examples&) = delete;
  Examples& operator=(const Examples&) = delete;
  size_t size() const { int64_t n = 0; agz::check(agz_examples_count(h, &n), "len(ex)"); return (size_t)n; }
  void Append(Arena& a) { agz::check(agz_examples_append_arena(h, a.h), "append(ex, SelfPlay()...)"); }
  void AugmentRotate() { agz::check(agz_examples_augment_rotate(h), "RotateBoard"); }
  void AugmentDihedral() { agz::check(agz_examples_augment_dihedral(h), "AugmentDihedral"); }   // all eight board symmetries, one pass
  int Prepare(int BatchSize, int maxExamples, uint64_t seed) {  // agogo.go:118-121 + prepareExamples
    int b = 0;
    agz::check(agz_examples_prepare(h, BatchSize, maxExamples, seed, &b), "prepareExamples");
    return b;
  }
};
// build extension: a sliding window over the most recent `capacity` examples, kept on the device across epochs (agz_replay): minibatches
// are drawn from it uniformly, each row under a random board symmetry applied as it is drawn (dual::TrainReplay)
struct Replay {
  agz_replay* h = nullptr;
  Replay(agz::Ctx& ctx, int F, int H, int W, int policyLen, int64_t capacity) {
    agz::check(agz_replay_create(ctx.h, F, H, W, policyLen, capacity, &h), "Replay");
  }
  // the planes kept as 2-bit codes under a palette of 1 to 4 bit patterns (agz_replay_create_packed): an append then takes all rows or none
  Replay(agz::Ctx& ctx, int F, int H, int W, int policyLen, int64_t capacity, const std::vector<float>& palette) {
    agz::check(agz_replay_create_packed(ctx.h, F, H, W, policyLen, capacity, palette.data(), (int)palette.size(), &h), "Replay");
  }
  // bytes of the ring on the device
  int64_t DeviceBytes() const { int64_t b = 0; agz::check(agz_replay_storage(h, nullptr, nullptr, &b), "window storage"); return b; }
  ~Replay() { agz_replay_destroy(h); }
  Replay(const Replay&) = delete;
  Replay& operator=(const Replay&) = delete;
  size_t size() const { int64_t n = 0; agz::check(agz_replay_count(h, &n, nullptr, nullptr), "len(window)"); return (size_t)n; }   // live rows
  void Append(Examples& ex) { agz::check(agz_replay_append_examples(h, ex.h), "append(window, ex...)"); }
  // Checkpoint of the window and the continuation from one (agz_replay_save / agz_replay_load): the live rows in logical order, total,
  // form and digest.  A file loads into a window of the same row shape, whatever its capacity and form; a bad file changes nothing.
  void Save(const std::string& path) { agz::check(agz_replay_save(h, path.c_str()), "Replay.Save"); }
  void Load(const std::string& path) { agz::check(agz_replay_load(h, path.c_str()), "Replay.Load"); }
  uint64_t Digest() const { uint64_t d = 0; agz::check(agz_replay_digest(h, &d), "window digest"); return d; }
};
// agogo.Config (datatypes.go:14-25)
struct Config {
  std::string Name;
  dual::Config NNConf;
  mcts::Config MCTSConf;
  double UpdateThreshold = 0.52;
  int MaxExamples = 0;
  int Encoder = AGZ_ENC_TWOPLANE;
  bool AugmentRotate = false;  // Augmenter (datatypes.go:24): the RotateBoard-based rotation augmenter, or none
  bool AugmentDihedral = false;  // build extension: the four rotations and the four reflections (takes precedence over AugmentRotate)
  // build extension: leaf symmetry of the self-play and evaluation arenas (Arena::SetLeafSymmetry); AGZ_SYM_OFF = the reference's search
  int LeafSymmetry = AGZ_SYM_OFF;
  // build extension: root noise of the SELF-PLAY arena (Arena::SetRootNoise): RootNoiseEps = 0 means off.  The evaluation arena that gates
  // a new network always plays without noise
  float RootNoiseEps = 0.f;
  float RootNoiseAlpha = 0.3f;
  // build extension: the arithmetic of the inference networks (agz_net_set_compute_mode) and, through it, of the trainer: AGZ_COMPUTE_F32_MFMA
  // (default), AGZ_COMPUTE_BF16X3, AGZ_COMPUTE_WINO (training then uses BF16X3), AGZ_COMPUTE_WINO_H2 / AGZ_COMPUTE_AUTO (the measured mode;
  // training takes the trainer's AGZ_COMPUTE_WINO_H2)
  int ComputeMode = AGZ_COMPUTE_F32_MFMA;
  // build extension: the options of the solver dual.Train builds (agz_trainer_set_solver); all 0 (default) = the reference's vanilla solver.
  // Applied to A, B and every newB.
  agz_solver_conf Solver = {0.f, 0.f, 0.f, 0};
  // build extension: the loss dual.Train optimises (agz_trainer_set_loss): AGZ_LOSS_REFERENCE (default) = the reference's, AGZ_LOSS_ALPHAZERO
  // = softmax cross-entropy and an MSE on tanh.  Applied with the solver options to A, B and every newB.  Like the kind in a trainer file,
  // it is not in a SaveRun file (AGZRUN01 unchanged): a resumed run trains under the Loss of the Config its AZ was constructed with.
  int Loss = AGZ_LOSS_REFERENCE;
  // build extension: the policy row the SELF-PLAY arena records (Arena::SetPolicyTarget): AGZ_TARGET_REFERENCE (default) = the reference's
  // Policies, AGZ_TARGET_VISITS = the root's visit distribution N(a)^(1/TargetTemperature), the target AGZ_LOSS_ALPHAZERO is meant for.  The
  // evaluation arena records nothing.  Like Loss, neither field is in a SaveRun file (AGZRUN01 unchanged)
  int PolicyTarget = AGZ_TARGET_REFERENCE;
  float TargetTemperature = 1.f;
  // build extension: playout cap randomization of the SELF-PLAY arena (Arena::SetPlayoutCap): PlayoutCapFastBudget = 0 (default) means off,
  // otherwise a ply is a full search of MCTSConf.Budget simulations with probability PlayoutCapFull and a fast one of PlayoutCapFastBudget
  // simulations — without root noise and without a recorded row — otherwise.  The evaluation arena always searches in full.  Like Loss and
  // PolicyTarget, neither field is in a SaveRun file (AGZRUN01 unchanged): a resumed run plays under the Config its AZ was constructed with
  int PlayoutCapFastBudget = 0;
  float PlayoutCapFull = 0.25f;
  // build extension: forced playouts of the SELF-PLAY arena (Arena::SetForcedPlayouts): ForcedPlayoutsK = 0 (default) means off, otherwise
  // a root child with n playouts and prior P is selected while n^2 < K P T (T the playouts below the root); ForcedPrune takes the forced
  // playouts of a move that turned out bad back out of the PolicyTarget = AGZ_TARGET_VISITS row.  With the playout cap only full plies
  // force.  The evaluation arena searches without them.  Neither field is in a SaveRun file (AGZRUN01 unchanged)
  float ForcedPlayoutsK = 0.f;
  bool ForcedPrune = true;
  // build extension: train from a replay window instead of one epoch's examples.  ReplayWindow = rows the window keeps across epochs; 0
  // (default) = off, AZ.Learn exactly as the reference has it.  ReplaySteps = minibatches per epoch; 0 = (live rows / BatchSize) * nniters.
  // ReplaySymmetric = every sampled row under one of the eight board symmetries, chosen per draw; the materialising augmenters
  // (AugmentRotate / AugmentDihedral) are then not applied.  MaxExamples is not applied either: the window is the cut.
  int64_t ReplayWindow = 0;
  int ReplaySteps = 0;
  bool ReplaySymmetric = false;
  // ReplayPacked = the window keeps its planes as 2-bit codes under agz_encoder_palette(Encoder): 8.8 times fewer bytes a row at 19x19,
  // the same bits sampled.  false (default) = the fp32 window, nothing changes.
  bool ReplayPacked = false;
  // test hooks (not in the reference): inferencers of the self-play games once the dummy is no longer in use, and of the evaluation
  // games — AGZ_INF_NET plays the networks as the reference does; the synthetic kinds make an epoch's games independent of fp32 rounding
  // in a network evaluation (tests/test_learn_parity_gpu.py compares the epoch log with oracle/learn.hpp)
  int SelfPlayInferencer[2] = {AGZ_INF_NET, AGZ_INF_NET};
  int EvalInferencer[2] = {AGZ_INF_NET, AGZ_INF_NET};
};
// Statistics (statistics.go:10-38): per network — keyed by its identity, the reference formats the pointer — the A side's Wins / Loss /
// Draw of every epoch in which it was A
struct Statistics {
  std::vector<int> Creation;
  std::map<int, std::vector<float>> Wins, Losses, Draws;
  void update(int a_id, float wins, float loss, float draw) {
    if (!Wins.count(a_id)) Creation.push_back(a_id);
    Wins[a_id].push_back(wins); Losses[a_id].push_back(loss); Draws[a_id].push_back(draw);
  }
};
struct GameSpec { int kind, m, n, k; float komi; };

// AZ (agogo.go:21-172): the trainer loop around the device hot path.  Self-play episodes and arena games of an epoch
// run concurrently as one batched arena each; everything else follows AZ.Learn line by line.
struct AZ {
  agz::Ctx& ctx;
  GameSpec game;
  Config conf;
  std::unique_ptr<dual::Trainable> A, B;      // Agent.NN (trainable, full shapes)
  std::unique_ptr<dual::Dual> infA, infB;     // SwitchToInference products (agent.go:42-57)
  bool useDummy = true;
  uint64_t seed;
  // (window, steps: the replay window's live rows after this epoch's append and the minibatches trained on; 0 without a window)
  struct EpochStats { int epoch; size_t examples; int batches; float cost; long a_wins, b_wins, draws; bool killedA; int a_id; size_t window; int steps; };
  std::unique_ptr<Replay> window;              // Config::ReplayWindow > 0: one window across epochs
  std::vector<EpochStats> log;
  Statistics stats;
  int a_id = 1, b_id = 2, next_id = 3;         // network identities (the reference's %p of Agent.NN)
  int epochs_done = 0;                         // the epoch the next Learn of a continued run starts at (SaveRun / LoadRun)

  AZ(agz::Ctx& c, GameSpec g, const Config& cf, uint64_t seed_ = 1337) : ctx(c), game(g), conf(cf), seed(seed_) {  // agogo.go:41-72
    if (!cf.NNConf.IsValid()) throw agz::Error("NNConf is not valid. Unable to proceed");
    if (!cf.MCTSConf.IsValid()) throw agz::Error("MCTSConf is not valid. Unable to proceed");
    A.reset(new dual::Trainable(ctx, cf.NNConf)); A->Init(seed * 3 + 1); applySolver(*A);
    B.reset(new dual::Trainable(ctx, cf.NNConf)); B->Init(seed * 3 + 2); applySolver(*B);
    infA.reset(new dual::Dual(ctx, cf.NNConf)); infB.reset(new dual::Dual(ctx, cf.NNConf));
    if (cf.ReplayWindow > 0 && cf.ReplayPacked) {
      float pal[4];
      int n = 0;
      agz::check(agz_encoder_palette(cf.Encoder, pal, &n), "encoder palette");
      window.reset(new Replay(ctx, cf.NNConf.Features, cf.NNConf.Height, cf.NNConf.Width, cf.NNConf.ActionSpace, cf.ReplayWindow,
                              std::vector<float>(pal, pal + n)));
    } else if (cf.ReplayWindow > 0) {
      window.reset(new Replay(ctx, cf.NNConf.Features, cf.NNConf.Height, cf.NNConf.Width, cf.NNConf.ActionSpace, cf.ReplayWindow));
    }
  }
  void applySolver(dual::Trainable& t) const {   // (the default options leave the trainer untouched: no call)
    if (conf.Solver.momentum != 0.f || conf.Solver.l2reg != 0.f || conf.Solver.clip != 0.f) t.SetSolver(conf.Solver.momentum, conf.Solver.l2reg, conf.Solver.clip);
    if (conf.Loss != AGZ_LOSS_REFERENCE) t.SetLoss(conf.Loss);
  }
  // AZ.Learn (agogo.go:100-172).  Build extension: epochs first_epoch .. first_epoch + iters - 1, each with the seeds epoch number `epoch`
  // has in an uninterrupted run, so Learn(2, ...), SaveRun, LoadRun on a new AZ and Learn(1, ..., 2) is Learn(3, ...).
  void Learn(int iters, int episodes, int nniters, int arenaGames, int first_epoch = 0) {
    for (int epoch = first_epoch; epoch < first_epoch + iters; epoch++) {
      EpochStats st{}; st.epoch = epoch;
      A->SwitchToInference(*infA); B->SwitchToInference(*infB);           // setupSelfPlay, agogo.go:75-90
      agz::check(agz_net_set_compute_mode(infA->h, conf.ComputeMode), "compute mode");
      agz::check(agz_net_set_compute_mode(infB->h, conf.ComputeMode), "compute mode");
      if (conf.ComputeMode == AGZ_COMPUTE_BF16X3 || conf.ComputeMode == AGZ_COMPUTE_WINO) B->SetComputeMode(AGZ_COMPUTE_BF16X3);
      else if (conf.ComputeMode == AGZ_COMPUTE_WINO_H2 || conf.ComputeMode == AGZ_COMPUTE_AUTO) B->SetComputeMode(AGZ_COMPUTE_WINO_H2);
      Examples ex(ctx, conf.NNConf.Features, conf.NNConf.Height, conf.NNConf.Width, conf.NNConf.ActionSpace);
      {
        Arena sp(ctx, game.kind, game.m, game.n, game.k, game.komi, conf.Encoder, conf.MCTSConf, episodes, seed + 1000 * epoch);
        if (epoch == 0 && useDummy) sp.SetAgents(nullptr, nullptr);
        else sp.SetAgentKinds(conf.SelfPlayInferencer[0], infA.get(), conf.SelfPlayInferencer[1], infB.get());
        if (conf.LeafSymmetry != AGZ_SYM_OFF) sp.SetLeafSymmetry(conf.LeafSymmetry, seed + 1000 * epoch + 1);
        if (conf.RootNoiseEps > 0.f) sp.SetRootNoise(conf.RootNoiseEps, conf.RootNoiseAlpha);
        if (conf.PolicyTarget != AGZ_TARGET_REFERENCE) sp.SetPolicyTarget(conf.PolicyTarget, conf.TargetTemperature);
        if (conf.PlayoutCapFastBudget > 0) sp.SetPlayoutCap(conf.PlayoutCapFull, conf.PlayoutCapFastBudget, seed + 1000 * epoch + 2);
        if (conf.ForcedPlayoutsK > 0.f) sp.SetForcedPlayouts(conf.ForcedPlayoutsK, conf.ForcedPrune);
        sp.PlayOnDevice(true);                                            // episodes x SelfPlay(), agogo.go:110-114
        ex.Append(sp);                                                     // device to device, episode after episode
      }
      const bool sampled_sym = window && conf.ReplaySymmetric;             // the sampler applies the symmetries: nothing is materialised
      if (conf.AugmentDihedral && !sampled_sym) ex.AugmentDihedral();
      else if (conf.AugmentRotate && !sampled_sym) ex.AugmentRotate();     // Arena.Play's aug(ex), arena.go:115-120
      st.examples = ex.size();
      if (window) {
        window->Append(ex);                                                // the epoch's examples join the window, the oldest rows leave it
        st.window = window->size();
        st.batches = (int)(st.window / (size_t)conf.NNConf.BatchSize);
        st.steps = conf.ReplaySteps > 0 ? conf.ReplaySteps : st.batches * nniters;
        if (st.steps == 0) throw agz::Error("batches is nil, probably too few examples regarding the batchsize");
        st.cost = dual::TrainReplay(*B, window->h, st.steps, seed + 17 * epoch, conf.ReplaySymmetric);
      } else {
        // maxExamples cut (agogo.go:118-121) + prepareExamples (agogo.go:211-249), tensors stay in HBM
        int batches = ex.Prepare(conf.NNConf.BatchSize, conf.MaxExamples, seed + 13 * epoch + 1);
        if (batches == 0) throw agz::Error("batches is nil, probably too few examples regarding the batchsize");  // agogo.go:123-125
        st.batches = batches;
        float *Xs = nullptr, *Pi = nullptr, *V = nullptr;
        agz::check(agz_examples_tensors_dev(ex.h, &Xs, &Pi, &V, nullptr, nullptr), "prepareExamples");
        st.cost = dual::TrainDev(*B, Xs, Pi, V, batches, nniters, seed + 17 * epoch);  // agogo.go:133
      }
      B->SwitchToInference(*infB);                                         // agogo.go:137
      {
        Arena ev(ctx, game.kind, game.m, game.n, game.k, game.komi, conf.Encoder, conf.MCTSConf, arenaGames, seed + 1000 * epoch + 500);
        ev.SetAgentKinds(conf.EvalInferencer[0], infA.get(), conf.EvalInferencer[1], infB.get());
        if (conf.LeafSymmetry != AGZ_SYM_OFF) ev.SetLeafSymmetry(conf.LeafSymmetry, seed + 1000 * epoch + 501);
        ev.Play(false);                                                   // agogo.go:144-148
        int64_t aw = 0, bw = 0, dr = 0;
        agz::check(agz_arena_get_results(ev.h, &aw, &bw, &dr), "results");
        st.a_wins = aw; st.b_wins = bw; st.draws = dr;
      }
      st.killedA = false;
      if (st.b_wins + st.a_wins > 0 && (float)st.b_wins / (float)(st.b_wins + st.a_wins) > (float)conf.UpdateThreshold) {  // agogo.go:155
        A = std::move(B); a_id = b_id;                                     // a.A.NN = a.B.NN
        st.killedA = true;
      }
      // a.update(a.A) (agogo.go:166, statistics.go:27-38): the A agent's wins / losses / draws of the evaluation games, under the name of
      // the network A holds NOW (B's, when A was killed)
      stats.update(a_id, (float)st.a_wins, (float)st.b_wins, (float)st.draws);
      st.a_id = a_id;
      b_id = next_id++;
      B.reset(new dual::Trainable(ctx, conf.NNConf));                      // newB: a fresh random net (arena.go:205-224)
      B->Init(seed * 3 + 100 + epoch);
      applySolver(*B);
      useDummy = useDummy && false;                                        // the dummy is only used in epoch 0 (agogo.go:83-87)
      log.push_back(st);
      epochs_done = epoch + 1;
    }
  }

  // ---- a run saved at an epoch boundary (build extension) ----------------------------------------------------------------------------
  // SaveRun(prefix) writes prefix + ".A" (A->Save: the trainer checkpoint of the network A holds), prefix + ".window" (window->Save, only
  // if there is a window) and, LAST, prefix + ".run", which is flushed, fsynced and renamed into place from a temporary file and names
  // the two files it belongs to: the length and an FNV-1a hash of the ".A" file's bytes, and the total and digest words of the ".window"
  // file.  The three files are not replaced together: a crash between two of them leaves a newer ".A" or ".window" beside the older
  // ".run", and LoadRun refuses that set, naming the file that does not match; the run is then lost back to the previous complete
  // SaveRun only if its files were kept under another prefix (alternate two prefixes to keep one complete set at all times).  B needs no
  // file: at every epoch boundary it is a fresh random network whose seed follows from `seed` and the epoch.  The ".run" file,
  // little-endian and unpadded:
  //
  //     "AGZRUN01"
  //     conf      uint32 n (= 45), float64 [n]: game kind, m, n, k, komi; NNConf K, SharedLayers, FC, L2, BatchSize, Width, Height, Features,
  //               ActionSpace, FwdOnly; MCTSConf PUCT, M, N, RandomCount, Budget, RandomMinVisits, RandomTemperature, DumbPass,
  //               ResignPercentage, PassPreference; UpdateThreshold, MaxExamples, Encoder, AugmentRotate, AugmentDihedral, LeafSymmetry,
  //               RootNoiseEps, RootNoiseAlpha, ComputeMode, Solver momentum, l2reg, clip; ReplayWindow, ReplaySteps, ReplaySymmetric,
  //               ReplayPacked; SelfPlayInferencer[2], EvalInferencer[2]   (every value is exact as a float64; compared bit by bit)
  //     state     uint64 seed, uint32 epochs_done, uint32 useDummy, int32 a_id, b_id, next_id, uint32 has_window
  //     files     uint64 bytes of the ".A" file, uint64 FNV-1a (64 bit) of them, uint64 total and uint64 digest of the ".window" file (its
  //               header words at byte offsets 48 and 72, csrc/replay_ckpt.hpp; 0, 0 without a window)
  //     stats     uint32 nets, then per network in Creation order: int32 id, uint32 n, float32 Wins[n], Losses[n], Draws[n]
  //     log       uint32 n, then per epoch: int32 epoch, uint64 examples, int32 batches, float32 cost, int64 a_wins, b_wins, draws,
  //               uint32 killedA, int32 a_id, uint64 window, int32 steps
  //     end       "AGZRUNZZ", uint64 the file's total length
  //
  // LoadRun(prefix), on a newly constructed AZ of the same game and Config: the ".run" file is read and checked WHOLE first — a malformed
  // one, one of another configuration (the message names the field), or one whose ".A" / ".window" files are not the ones it was written
  // beside throws before anything is loaded.  Then the ".A" file is loaded into a NEW trainer and the window file into the window
  // (agz_replay_load: a bad file changes nothing); only when both have succeeded does the new trainer become A, with the solver options
  // applied again (l2reg and clip are not in a trainer file), are the fields above restored and is B rebuilt exactly as the end of epoch
  // epochs_done - 1 builds it.  A failure anywhere leaves the AZ as it was.
  static void fileHash(const std::string& path, uint64_t* bytes, uint64_t* fnv) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw agz::Error("cannot open " + path);
    std::vector<unsigned char> buf(1 << 20);
    uint64_t d = 0xcbf29ce484222325ull, n = 0;
    for (size_t got; (got = fread(buf.data(), 1, buf.size(), f)) > 0; n += got)
      for (size_t i = 0; i < got; i++) d = (d ^ buf[i]) * 0x100000001b3ull;
    fclose(f);
    *bytes = n; *fnv = d;
  }
  static void windowWords(const std::string& path, uint64_t* total, uint64_t* digest) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw agz::Error("cannot open " + path);
    const bool ok = fseek(f, 48, SEEK_SET) == 0 && fread(total, 8, 1, f) == 1 && fseek(f, 72, SEEK_SET) == 0 && fread(digest, 8, 1, f) == 1;
    fclose(f);
    if (!ok) throw agz::Error(path + " is shorter than a window checkpoint's header");
  }
  std::vector<std::pair<const char*, double>> runConf() const {
    const dual::Config& n = conf.NNConf;
    const mcts::Config& m = conf.MCTSConf;
    return {{"game.kind", game.kind}, {"game.m", game.m}, {"game.n", game.n}, {"game.k", game.k}, {"game.komi", game.komi},
            {"NNConf.K", n.K}, {"NNConf.SharedLayers", n.SharedLayers}, {"NNConf.FC", n.FC}, {"NNConf.L2", n.L2}, {"NNConf.BatchSize", n.BatchSize},
            {"NNConf.Width", n.Width}, {"NNConf.Height", n.Height}, {"NNConf.Features", n.Features}, {"NNConf.ActionSpace", n.ActionSpace},
            {"NNConf.FwdOnly", n.FwdOnly}, {"MCTSConf.PUCT", m.PUCT}, {"MCTSConf.M", m.M}, {"MCTSConf.N", m.N}, {"MCTSConf.RandomCount", m.RandomCount},
            {"MCTSConf.Budget", m.Budget}, {"MCTSConf.RandomMinVisits", m.RandomMinVisits}, {"MCTSConf.RandomTemperature", m.RandomTemperature},
            {"MCTSConf.DumbPass", m.DumbPass}, {"MCTSConf.ResignPercentage", m.ResignPercentage}, {"MCTSConf.PassPreference", m.PassPreference},
            {"UpdateThreshold", conf.UpdateThreshold}, {"MaxExamples", conf.MaxExamples}, {"Encoder", conf.Encoder},
            {"AugmentRotate", conf.AugmentRotate}, {"AugmentDihedral", conf.AugmentDihedral}, {"LeafSymmetry", conf.LeafSymmetry},
            {"RootNoiseEps", conf.RootNoiseEps}, {"RootNoiseAlpha", conf.RootNoiseAlpha}, {"ComputeMode", conf.ComputeMode},
            {"Solver.momentum", conf.Solver.momentum}, {"Solver.l2reg", conf.Solver.l2reg}, {"Solver.clip", conf.Solver.clip},
            {"ReplayWindow", (double)conf.ReplayWindow}, {"ReplaySteps", conf.ReplaySteps}, {"ReplaySymmetric", conf.ReplaySymmetric},
            {"ReplayPacked", conf.ReplayPacked}, {"SelfPlayInferencer[0]", conf.SelfPlayInferencer[0]},
            {"SelfPlayInferencer[1]", conf.SelfPlayInferencer[1]}, {"EvalInferencer[0]", conf.EvalInferencer[0]},
            {"EvalInferencer[1]", conf.EvalInferencer[1]}};
  }
  void SaveRun(const std::string& prefix) {
    A->Save(prefix + ".A");
    if (window) window->Save(prefix + ".window");
    std::string b = "AGZRUN01";
    auto put = [&b](const auto& v) { b.append(reinterpret_cast<const char*>(&v), sizeof(v)); };
    const auto cw = runConf();
    put((uint32_t)cw.size());
    for (const auto& w : cw) put(w.second);
    put((uint64_t)seed); put((uint32_t)epochs_done); put((uint32_t)(useDummy ? 1 : 0));
    put((int32_t)a_id); put((int32_t)b_id); put((int32_t)next_id); put((uint32_t)(window ? 1 : 0));
    uint64_t files[4] = {0, 0, 0, 0};
    fileHash(prefix + ".A", &files[0], &files[1]);
    if (window) windowWords(prefix + ".window", &files[2], &files[3]);
    for (uint64_t w : files) put(w);
    put((uint32_t)stats.Creation.size());
    for (int id : stats.Creation) {
      const std::vector<float>&w = stats.Wins.at(id), &l = stats.Losses.at(id), &d = stats.Draws.at(id);
      put((int32_t)id); put((uint32_t)w.size());
      for (const std::vector<float>* v : {&w, &l, &d}) b.append(reinterpret_cast<const char*>(v->data()), v->size() * 4);
    }
    put((uint32_t)log.size());
    for (const EpochStats& e : log) {
      put((int32_t)e.epoch); put((uint64_t)e.examples); put((int32_t)e.batches); put((float)e.cost); put((int64_t)e.a_wins); put((int64_t)e.b_wins);
      put((int64_t)e.draws); put((uint32_t)(e.killedA ? 1 : 0)); put((int32_t)e.a_id); put((uint64_t)e.window); put((int32_t)e.steps);
    }
    b += "AGZRUNZZ";
    put((uint64_t)(b.size() + 8));
    const std::string path = prefix + ".run", tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) throw agz::Error("AZ.SaveRun: cannot open " + tmp);
    const bool written = fwrite(b.data(), 1, b.size(), f) == b.size() && fflush(f) == 0 && fsync(fileno(f)) == 0;
    const bool closed = fclose(f) == 0;
    if (!(written && closed && rename(tmp.c_str(), path.c_str()) == 0)) {
      remove(tmp.c_str());
      throw agz::Error("AZ.SaveRun: cannot write " + path);
    }
  }
  void LoadRun(const std::string& prefix) {
    const std::string path = prefix + ".run";
    std::string b;
    {
      FILE* f = fopen(path.c_str(), "rb");
      if (!f) throw agz::Error("AZ.LoadRun: cannot open " + path);
      char buf[4096];
      for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) b.append(buf, n);
      fclose(f);
    }
    size_t at = 0;
    auto bad = [&path](const std::string& why) { return agz::Error("AZ.LoadRun: " + path + " is malformed: " + why); };
    auto get = [&](auto& v) {
      if (b.size() - at < sizeof(v)) throw bad("truncated");
      memcpy(&v, b.data() + at, sizeof(v));
      at += sizeof(v);
    };
    if (b.size() < 24 || b.compare(0, 8, "AGZRUN01") != 0) throw bad("not a run file (magic)");
    uint64_t length = 0;
    memcpy(&length, b.data() + b.size() - 8, 8);
    if (b.compare(b.size() - 16, 8, "AGZRUNZZ") != 0 || length != b.size()) throw bad("bad end marker (truncated or overlong)");
    at = 8;
    const auto cw = runConf();
    uint32_t n = 0;
    get(n);
    if (n != cw.size()) throw bad("it holds " + std::to_string(n) + " configuration words, this build writes " + std::to_string(cw.size()));
    for (const auto& w : cw) {
      double v = 0;
      get(v);
      if (memcmp(&v, &w.second, 8) != 0)
        throw agz::Error("AZ.LoadRun: " + path + " belongs to another configuration: " + w.first + " is " + std::to_string(v) + " in the file, " +
                         std::to_string(w.second) + " here");
    }
    uint64_t seed_ = 0;
    uint32_t done = 0, dummy = 0, has_window = 0, nets = 0, entries = 0;
    int32_t ia = 0, ib = 0, inext = 0;
    get(seed_); get(done); get(dummy); get(ia); get(ib); get(inext); get(has_window);
    if (dummy > 1 || has_window > 1 || done > 0x7fffffffu) throw bad("a flag or the epoch count is out of range");
    if ((has_window != 0) != (window != nullptr)) throw bad("it was written with" + std::string(has_window ? "" : "out") + " a replay window");
    uint64_t files[4] = {0, 0, 0, 0};
    for (uint64_t& w : files) get(w);
    Statistics st;
    get(nets);
    for (uint32_t i = 0; i < nets; i++) {
      int32_t id = 0;
      uint32_t cnt = 0;
      get(id); get(cnt);
      if ((b.size() - at) / 12 < cnt || st.Wins.count(id)) throw bad("statistics");
      st.Creation.push_back(id);
      for (std::vector<float>* v : {&st.Wins[id], &st.Losses[id], &st.Draws[id]}) {
        v->resize(cnt);
        if (cnt) memcpy(v->data(), b.data() + at, (size_t)cnt * 4);
        at += (size_t)cnt * 4;
      }
    }
    std::vector<EpochStats> lg;
    get(entries);
    for (uint32_t i = 0; i < entries; i++) {
      EpochStats e{};
      int32_t epoch = 0, batches = 0, id = 0, steps = 0;
      uint64_t examples = 0, win = 0;
      int64_t aw = 0, bw = 0, dr = 0;
      uint32_t killed = 0;
      get(epoch); get(examples); get(batches); get(e.cost); get(aw); get(bw); get(dr); get(killed); get(id); get(win); get(steps);
      if (killed > 1) throw bad("log");
      e.epoch = epoch; e.examples = (size_t)examples; e.batches = batches; e.a_wins = (long)aw; e.b_wins = (long)bw; e.draws = (long)dr;
      e.killedA = killed != 0; e.a_id = id; e.window = (size_t)win; e.steps = steps;
      lg.push_back(e);
    }
    if (at + 16 != b.size()) throw bad("bytes between the log and the end marker");
    // the ".A" and ".window" files are the ones this ".run" was written beside
    uint64_t have[4] = {0, 0, 0, 0};
    fileHash(prefix + ".A", &have[0], &have[1]);
    if (have[0] != files[0] || have[1] != files[1])
      throw agz::Error("AZ.LoadRun: " + prefix + ".A is not the trainer file " + path + " was written beside (another length or hash: a SaveRun that did not finish?)");
    if (window) {
      windowWords(prefix + ".window", &have[2], &have[3]);
      if (have[2] != files[2] || have[3] != files[3])
        throw agz::Error("AZ.LoadRun: " + prefix + ".window is not the window file " + path + " was written beside (another total or digest: a SaveRun that did not finish?)");
    }
    // the set is sound and of this configuration: from here on things are loaded, A into a new trainer so that a failure changes nothing
    std::unique_ptr<dual::Trainable> loaded(new dual::Trainable(ctx, conf.NNConf));
    loaded->Load(prefix + ".A");
    applySolver(*loaded);
    if (window) window->Load(prefix + ".window");
    A = std::move(loaded);
    seed = seed_; epochs_done = (int)done; useDummy = dummy != 0; a_id = ia; b_id = ib; next_id = inext;
    stats = st; log = lg;
    if (epochs_done > 0) {
      B.reset(new dual::Trainable(ctx, conf.NNConf));
      B->Init(seed * 3 + 100 + (uint64_t)(epochs_done - 1));
      applySolver(*B);
    }
  }
};
}  // namespace agogo
