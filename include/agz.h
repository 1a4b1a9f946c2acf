/*
 * agz.h — C ABI of libagz.so: the MI355X-native replacement for agogo's self-play hot path.
 *
 * Everything here is plain C (opaque handles, plain pointers and sizes, int error codes); no C++
 * or torch types cross this boundary.  Each entry point cites the reference interface it
 * replaces (paths are relative to the gorgonia/agogo tree).  The cgo binding a maintainer would
 * add on the reference side is in INTEGRATION.md / go/agzhip.
 *
 * Threading: an agz_ctx owns one HIP device + one stream and is NOT thread-safe (reference:
 * under `-tags cuda` agogo serialises on a single VM, const_cuda.go:5).  Drive one ctx from one
 * OS thread (Go: runtime.LockOSThread); different ctxs may be driven concurrently.
 *
 * Ownership: the caller allocates every output buffer; the library never returns interior
 * pointers (the reference's Inferencer.Infer returns a slice aliasing the VM output,
 * dualnet/meta.go:186-189 — a latent race this ABI does not reproduce).
 *
 * Errors: 0 = ok, <0 = AGZ_E_*; agz_last_error() returns a thread-local message.
 *
 * Environment switches (ALL of them; each is read once per process, the API default applies when unset, and
 * each has a test that runs it against the default — named in brackets):
 *   AGZ_RCCL_LIB=<path>       library dlopen'ed for the ncclXxx symbols instead of librccl.so (agz_comm_*)
 *                             [tests/test_comm_fake_gpu.py, tests/test_train_gpu.py: the in-tree fake RCCL]
 *   AGZ_WINO_H2_TM=4|5        Winograd tile of AGZ_COMPUTE_WINO_H2: F(4x4,3x3) / F(5x5,3x3); default: the one with
 *                             fewer transform-domain rows for the board   [tests/test_wino_gpu.py knobs test]
 *   AGZ_WINO_H2_CHUNK=<n>     boards per chunk of the AGZ_COMPUTE_WINO_H2 tower (default: as many as 32-bit
 *                             offsets allow); results are bit-identical  [tests/test_wino_gpu.py knobs test]
 *   AGZ_WINO_H2_QUEUES=1|2    overrides agz_net_set_tower_queues         [tests/test_wino_gpu.py knobs test]
 *   AGZ_WINO_H2_FORM=0        the three-kernel block (in / GEMM / out) instead of the chained one (out of block l + in of
 *                             block l+1 in one kernel); same tolerance       [tests/test_wino_gpu.py knobs test]
 *   AGZ_WINO_H2_GEMM=1|2      the GEMM kernel of the chained AGZ_COMPUTE_WINO_H2 block: 1 = 128 x 256 tiles, both operands streamed,
 *                             three workgroups per CU (default); 2 = persistent, the weight slab stationary in registers (K = 256);
 *                             + 64: M / V2c stored with the default cache policy instead of non-temporally (round 4's behaviour);
 *                             + 128: every transform-domain row kept, also those that only feed off-board outputs (agz_debug.h);
 *                             all bit-identical                          [tests/test_wino_gpu.py knobs test]
 *   AGZ_WINO_CHUNK=<n>        boards per chunk of the AGZ_COMPUTE_WINO tower; bit-identical
 *                             [tests/test_wino_gpu.py::test_wino_board_chunks_in_a_subprocess]
 */
#ifndef AGZ_H
#define AGZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGZ_OK 0
#define AGZ_E_INVALID (-1)   /* bad argument / invalid config (reference: Config.IsValid, agogo.go:42-47 panics) */
#define AGZ_E_HIP (-2)       /* HIP runtime failure */
#define AGZ_E_NOMEM (-3)
#define AGZ_E_STATE (-4)     /* call sequence error (e.g. infer before commit) */
#define AGZ_E_TREE_FULL (-5) /* a tree's node pool overflowed (reference cap: MAXTREESIZE, mcts/search.go:23) */
#define AGZ_E_UNSUPPORTED (-6)
#define AGZ_E_CALLBACK (-8)  /* a host inferencer (AGZ_INF_CALLBACK) returned non-zero: the search was aborted */
#define AGZ_E_PEER (-7)      /* a data-parallel step failed on ANOTHER rank (agz_trainer_forward_backward_allreduce): gradients undefined */

typedef struct agz_ctx agz_ctx;
typedef struct agz_net agz_net;
typedef struct agz_arena agz_arena;

/* game.Colour / game.Player values (game/state.go:9-13) */
#define AGZ_NONE 0
#define AGZ_BLACK 1
#define AGZ_WHITE 2
/* game.Single special moves (mcts/mcts.go:21-22) */
#define AGZ_PASS (-1)
#define AGZ_RESIGN (-2)

const char* agz_last_error(void);
/* library / build info string ("libagz <ver> gfx950 ...") */
const char* agz_version(void);

/* ---- context ------------------------------------------------------------------------------ */
/* One HIP device + stream.  Replaces the implicit gorgonia VM/engine an Agent owns (agent.go:44-53). */
int agz_ctx_create(int device, agz_ctx** out);
void agz_ctx_destroy(agz_ctx* ctx);
/* Page-locked host memory for the buffers handed to the host-pointer entry points (agz_net_infer, agz_arena_get_*, ...):
 * the library stages pageable memory through the driver's bounce buffer; a buffer from agz_host_alloc is DMA-ed directly
 * (the batch-1 agogo.Inferer path — agent.go:60-74 hands one board per call — is pure latency otherwise).  Plain host
 * memory as far as the caller is concerned; free with agz_host_free before the ctx goes. */
int agz_host_alloc(agz_ctx* ctx, size_t bytes, void** out);
int agz_host_free(agz_ctx* ctx, void* p);
int agz_ctx_sync(agz_ctx* ctx);
/* raw hipStream_t the ctx launches on (for callers that want to record their own events) */
void* agz_ctx_stream(agz_ctx* ctx);
/* (kernel-class timers and test diagnostics: include/agz_debug.h — not part of the drop-in surface) */
/* ---- dual network ------------------------------------------------------------------------- */
/* Fields 1:1 with dual.Config (dualnet/config.go:4-16); bn_* pin the BatchNorm inference
 * semantics that live in un-vendored gorgonia. */
#define AGZ_BN_DEGENERATE_EPS 0 /* x / sqrt(0 + eps) * gamma + beta  (op.Reset() before every Infer, meta.go:170-172) */
#define AGZ_BN_RUNNING 1        /* (x - mean_c) / sqrt(var_c + eps) * gamma + beta, stats via agz_net_set_bn_stats */
#define AGZ_BN_IDENTITY 2       /* x * gamma + beta */
typedef struct agz_net_conf {
  int32_t K;            /* filters */
  int32_t SharedLayers; /* dual-branch blocks */
  int32_t FC;           /* value hidden width */
  int32_t BatchSize;    /* only used for Glorot fan computation of batch-shaped params (App. B b5) */
  int32_t Width, Height;
  int32_t Features;
  int32_t ActionSpace;  /* policy width (moves + pass) */
  int32_t bn_mode;      /* AGZ_BN_* */
  float bn_eps;         /* 1e-5 in the reference (ermahagerdmonards.go:54) */
} agz_net_conf;

/* dual.New + (*Dual).Init (dualnet/dual.go:33-47). Parameters are created zeroed. */
int agz_net_create(agz_ctx* ctx, const agz_net_conf* conf, agz_net** out);
void agz_net_destroy(agz_net* net);
/* (*Dual).Model() (dualnet/dual.go:134-142): learnables in creation order of Dual.fwd:
 *   Init{filter,gamma,beta}, per shared layer {L1 filter,gamma,beta, L2 filter,gamma,beta},
 *   PolicyHead{filter,gamma,beta}, Policy_w, Policy_b, ValueHead{filter,gamma,beta}, Value_w, Value_b,
 *   ValueOutput_w, ValueOutput_b.
 * Row-0 shapes are stored: conv filter [out,in,k,k]; BN gamma/beta [C,H,W]; FC w [in,units]; FC b [units]. */
int agz_net_num_params(const agz_net* net);
int agz_net_param_info(const agz_net* net, int index, char* name, size_t name_cap, size_t* n_elems);
/* G.Let on a learnable / the copy loop of dual.Infer (dualnet/meta.go:141-146).  n may exceed the
 * row-0 size (batch-shaped reference tensors): the first n_elems floats (= row 0) are taken, as Go
 * copy() + "only row 0 is ever real" does (App. B b5).  For BN params n == C broadcasts per channel. */
int agz_net_set_param(agz_net* net, int index, const float* host, size_t n);
int agz_net_get_param(const agz_net* net, int index, float* host, size_t n);
/* per-channel running statistics for AGZ_BN_RUNNING; bn_index counts BN ops in Dual.ops order
 * (dual.go:59-100: Init, L1/L2 of each shared layer, then policy, value). */
int agz_net_set_bn_stats(agz_net* net, int bn_index, const float* mean, const float* var, size_t C);
/* Random init with the reference's initialiser KINDS (GlorotU conv, GlorotN FC + BN gamma/beta,
 * zero FC bias; ermahagerdmonards.go:39,80,82) from the build's own RNG (Go's math/rand stream is
 * not reproducible here). */
int agz_net_init_random(agz_net* net, uint64_t seed);
/* Upload + repack to device layouts (folds BN into per-(c,h,w) scale/shift). Must follow any set_param. */
int agz_net_commit(agz_net* net);
/* dual.Infer + (*Inferencer).Infer (dualnet/meta.go:125-190), batched: planes [B,F,H,W] fp32 NCHW
 * (every board evaluated with row-0 parameters), policy [B,ActionSpace] softmax, value [B] tanh.
 * Host buffers (pageable ok). */
int agz_net_infer(agz_net* net, const float* planes, int B, float* policy, float* value);
/* same with device pointers, asynchronous on the ctx stream */
int agz_net_infer_dev(agz_net* net, const float* planes_dev, int B, float* policy_dev, float* value_dev);
/* Small-batch ("latency") regime for tournament-style single-tree Agent.Search (agent.go:76-81: one board per
 * Infer call): when a forward's tower would occupy <= 1/4 of the CUs, the convolutions run split-K and the heads are
 * spread over the chip.  On by default.  Within a regime results are bit-identical for every batch size; ACROSS the
 * two regimes the fp32 summation order differs (same tolerance vs the reference).  In AGZ_COMPUTE_F32_MFMA (the default mode)
 * the small-batch tower stays on exact fp32 products (split-K); in every other mode (AGZ_COMPUTE_AUTO included) K = 64 / 128 /
 * 256 towers take the one-launch-per-layer kernel with fp16x2 products on equilibrated operands (hi/lo fp16 pieces, the lo*lo
 * term of 2^-22 relative dropped; conv_lat.hpp) — same tolerance, 2.6x faster per layer at batch 1.  Turn the regime off for
 * strict bitwise batch-size independence at every batch size. */
int agz_net_set_latency_mode(agz_net* net, int on);
/* Queues the Winograd fp16x2 tower (AGZ_COMPUTE_WINO_H2) runs on: 2 = the batch is split into two halves whose block chains
 * run on two HIP streams, so one half's HBM-bound transform kernels run under the other half's GEMM (boards are independent:
 * results are bit-identical to one queue); 1 = one launch chain over the whole batch; 0 = auto (two queues from 256 boards
 * on, the default).  Per-kernel durations inflate under the overlap: measure kernels with 1. */
int agz_net_set_tower_queues(agz_net* net, int queues);
/* Arithmetic of the dual-block convolutions (both are fp32-grade and meet the same parity tolerance):
 *   AGZ_COMPUTE_F32_MFMA  v_mfma_f32_32x32x2_f32, exact fp32 products (default)
 *   AGZ_COMPUTE_BF16X3    every fp32 operand split exactly into three bf16 pieces, six bf16 MFMAs per product
 *                         (dropped cross terms <= 2^-23 relative), fp32 accumulation — 2.67x the fp32 matrix rate.
 *   AGZ_COMPUTE_FP16X2    every operand scaled by a power of two into fp16 range and split into two fp16 pieces
 *                         (23 significand bits), three fp16 MFMAs per product, fp32 accumulation; the scale of
 *                         every board's activations is measured on the device per layer (results stay independent
 *                         of the batch composition).  Same parity tolerance on the tested nets; elements more than
 *                         2^17 below their board's maximum lose relative precision — opt-in.
 *                         Both split modes apply to K a multiple of 64 and batches whose 128-row tiles fill the chip
 *                         (>= one tile per CU); other shapes keep F32_MFMA, which is faster there. */
#define AGZ_COMPUTE_F32_MFMA 0
#define AGZ_COMPUTE_BF16X3 1
#define AGZ_COMPUTE_FP16X2 2
#define AGZ_COMPUTE_WINO 3 /* Winograd F(4x4,3x3): transforms in fp32, the 36 transform-domain GEMMs with BF16X3 products — 3.6x
                            * fewer matrix instructions on 19x19; rounding error ~5x a direct fp32 convolution's (still inside
                            * the stated tolerance); opt-in, same shape conditions as the split modes */
#define AGZ_COMPUTE_AUTO 4 /* the measured choice: WINO_H2 where its weight image exists (K a multiple of 64), else BF16X3 where the
                            * split kernels apply, else F32_MFMA   [tests/test_wino_gpu.py::test_compute_auto_takes_the_measured_mode] */
#define AGZ_COMPUTE_WINO_H2 5 /* Winograd F(5x5,3x3) / F(4x4,3x3) (whichever needs fewer rows for the board) with FP16X2 products in the transform domain: the input transform writes the
                            * operand already split into two fp16 pieces (scaled per board by a power of two from a proven bound,
                            * overflow impossible), three fp16 MFMAs per product — half the matrix instructions of AGZ_COMPUTE_WINO */
#define AGZ_COMPUTE_FORCE 0x100 /* OR-ed in: take the split kernel even below the chip-filling threshold (tests) */
int agz_net_set_compute_mode(agz_net* net, int mode);
/* Checkpoint of the learnables in Model() order (+ BN statistics).  The reference gob-encodes G.Values
 * (AZ.Save / Dual.GobEncode, agogo.go:175-209, dualnet/dual.go:180-206); gob is Go-only, so this is a documented
 * flat format: "AGZNET01", agz_net_conf, n_params, then per parameter {uint64 n, float32[n]}, then per BN op
 * {uint64 C, mean[C], var[C]}.  agz_net_load requires an identical conf and leaves the net committed. */
int agz_net_save(const agz_net* net, const char* path);
int agz_net_load(agz_net* net, const char* path);
/* FLOPs of one evaluation (SURVEY App. D formula) */
double agz_net_flops_per_eval(const agz_net* net);

/* ---- dual.Train ---------------------------------------------------------------------- */
typedef struct agz_trainer agz_trainer;
/* The training graph of Dual.fwd + Dual.bwd (dualnet/dual.go:50-132) for conf->BatchSize rows.  Learnables keep the
 * reference's FULL shapes in Model() order: conv filter [out,in,k,k]; BN gamma/beta [B,C,H,W]; FC w [in,units];
 * FC b [B,units]  (batch-shaped).  BatchNorm runs in training mode (batch statistics). */
int agz_trainer_create(agz_ctx* ctx, const agz_net_conf* conf, agz_trainer** out);
/* Tied affine (opt-in; DESIGN §2 `tied-affine`): the same learnables in the same Model() order, but every batch-shaped one is stored ONCE,
 * at its row-0 shape — BatchNorm gamma / beta [C,H,W], Policy_b / Value_b / ValueOutput_b [units] — and shared by every row of a step:
 * agz_trainer_param_info returns exactly agz_net_param_info's sizes, and agz_trainer_export copies the whole trained state (nothing of
 * it is dropped, where a plain trainer exports row 0 of BatchSize independently trained copies).  Declared definition: forward and cost
 * are those of the plain trainer whose batch-shaped tensors hold the tied tensor in every row; the gradient of a tied tensor is the sum
 * over the batch rows of that plain trainer's per-row gradients (accumulated in double in row order, rounded once: no atomics,
 * reproducible to the bit); the solver step of the configured kind (vanilla, L2 / clip, momentum, Adam) is applied to the tied tensor
 * once, with that sum.  conf->BatchSize stays the number of rows of a step; it also still feeds the Glorot fans of
 * agz_trainer_init_random, so that a tied trainer draws row 0 of what a plain trainer of the same conf and seed draws.  Every entry
 * point of a plain trainer works on a tied handle (velocity and moments take the tied shapes; agz_trainer_allreduce reduces the now
 * small flat buffer in one call), except agz_trainer_forward_backward_allreduce(_dev), which return AGZ_E_STATE; the sharded
 * form is agz_trainer_create_sharded_tied below.  Checkpoints are "AGZTRN05" (agz_trainer_save below) and load only into a tied trainer.  A trainer made by
 * agz_trainer_create / agz_trainer_create_sharded runs exactly the kernels it ran before this option existed. */
int agz_trainer_create_tied(agz_ctx* ctx, const agz_net_conf* conf, agz_trainer** out);
int agz_trainer_is_tied(const agz_trainer* t, int* tied);   /* *tied = 1 for a handle of agz_trainer_create_tied, else 0 */
void agz_trainer_destroy(agz_trainer* t);
int agz_trainer_num_params(const agz_trainer* t);
int agz_trainer_param_info(const agz_trainer* t, int index, char* name, size_t name_cap, size_t* n_elems);
int agz_trainer_set_param(agz_trainer* t, int index, const float* host, size_t n);
int agz_trainer_get_param(const agz_trainer* t, int index, float* host, size_t n);
int agz_trainer_get_grad(const agz_trainer* t, int index, float* host, size_t n);
int agz_trainer_init_random(agz_trainer* t, uint64_t seed);
/* One batch of dual.Train's inner loop (dualnet/meta.go:33-40): Let planes/Pi/V, RunAll, solver.Step(lr).
 * planes [B,F,H,W], pi [B,ActionSpace], v [B] host buffers; *cost = xent(logits,Pi) + mean((o-V)^2) (dual.go:113-121).
 * NOTE (gradient read-back): with lr != 0 this call — and agz_train / agz_train_dev, which are loops of it — takes the SGD step of the
 * tower's batch-shaped gamma / beta INSIDE the BatchNorm backward kernel (98 % of the learnables: no gradient round trip), so their
 * gradients are NOT materialised: agz_trainer_get_grad / agz_trainer_grads_dev then return what an earlier forward_backward left there
 * for those tensors (zeros on a fresh trainer); filter and head gradients are current.  To read every gradient, run
 * agz_trainer_forward_backward (or agz_trainer_batch with lr = 0).  A step that fails part-way may have stepped some layers' gamma / beta
 * already: treat the trainer's parameters — and, with a momentum set (agz_trainer_set_solver), the velocity, which the same kernel steps —
 * as undefined after an error (reload a checkpoint, agz_trainer_load).  With Adam on (agz_trainer_set_adam) the same holds for the two
 * moments, which that kernel steps as well, and for the step counter t: both are undefined after a step that fails part-way. */
int agz_trainer_batch(agz_trainer* t, const float* planes, const float* pi, const float* v, float lr, float* cost);
/* Split form for data-parallel training: forward_backward fills the flat gradient buffer; all-reduce it over RCCL
 * (agz_trainer_grads_dev gives the device pointer: ONE collective per step); apply does w -= lr*grad_scale*grad. */
int agz_trainer_forward_backward(agz_trainer* t, const float* planes, const float* pi, const float* v, float* cost);
/* the same on device buffers (e.g. one batch of agz_examples_tensors_dev); cost may be NULL (no synchronisation) */
int agz_trainer_forward_backward_dev(agz_trainer* t, const float* planes_dev, const float* pi_dev, const float* v_dev, float* cost);
int agz_trainer_apply(agz_trainer* t, float lr, float grad_scale);
int agz_trainer_grads_dev(agz_trainer* t, float** dev_ptr, size_t* n_floats);
/* Solver options: what the reference chooses in its solver constructor, gorgonia.NewVanillaSolver(WithLearnRate(0.1)) (dualnet/meta.go:20)
 * — WithL2Reg, WithClip, or NewMomentum in its place.  Per learnable element, in fp32, with the per-call lr and grad_scale
 * (grad_scale is 1 on the fused path of agz_trainer_batch / agz_train / agz_train_dev):
 *     g1 = grad_scale * g
 *     g2 = g1 + l2reg * w                  (only if l2reg != 0)
 *     g3 = min(max(g2, -clip), clip)       (only if clip > 0)
 *     momentum == 0:  w = w + (-lr) * g3
 *     momentum != 0:  v = momentum * v + (-lr) * g3;  w = w + v        (v starts at 0)
 * L2 and clip apply to every learnable of Model(), the batch-shaped gamma / beta and FC biases included.  All options 0 (the default)
 * is the vanilla step: every path then runs exactly the kernels it ran before these options existed.  With any option set,
 * agz_trainer_batch still steps the tower's gamma / beta (and their velocity) inside the BatchNorm backward kernel; agz_trainer_apply
 * honours grad_scale on the two-pass and data-parallel paths.  The velocity is one device buffer the size of the learnables (7.7 GB at
 * 19x19 / K = 256 / 20 blocks / batch 256), allocated and zeroed when a momentum != 0 is first set (AGZ_E_NOMEM if it does not fit; the
 * options are then unchanged) and released when the momentum is set back to 0.  Note that a momentum step with lr = 0 still moves the
 * parameters by momentum * v: read gradients with agz_trainer_forward_backward.  Sharded trainers: every rank sets the same options
 * (a local call); a rank holds the velocity rows of the batch-shaped tensors it owns, the shared tensors' velocity is computed
 * identically on every rank from the summed gradient — no further collective.
 * set: AGZ_E_INVALID unless 0 <= momentum < 1, l2reg >= 0, clip >= 0, all finite and reserved == 0; the options stay as they were.
 * Tests: tests/test_solver_cpu.py (ABI), tests/test_solver_gpu.py (recurrence, fused = two-pass, oracle trajectory, validation). */
typedef struct agz_solver_conf { float momentum, l2reg, clip; int32_t reserved; } agz_solver_conf; /* 16 bytes, reserved = 0 */
int agz_trainer_set_solver(agz_trainer* t, const agz_solver_conf* conf);
int agz_trainer_get_solver(const agz_trainer* t, agz_solver_conf* out);
/* The velocity of learnable `index` (gorgonia's Momentum keeps one `cached` value per learnable; the reference never reads it): the
 * indexing, shapes and — on a sharded trainer — row ownership of agz_trainer_get_param.  get: zeros while no velocity exists
 * (momentum 0).  set: AGZ_E_STATE while no velocity exists.  Tests: test_solver_gpu.py (recurrence, checkpoint), test_solver_sharded_gpu.py. */
int agz_trainer_get_velocity(const agz_trainer* t, int index, float* host, size_t n);
int agz_trainer_set_velocity(agz_trainer* t, int index, const float* host, size_t n);
/* velocity := 0, the options kept (a fresh gorgonia solver with the same options).  Test: test_solver_gpu.py (checkpoint case). */
int agz_trainer_reset_solver(agz_trainer* t);
/* Adam: gorgonia.NewAdamSolver in place of NewVanillaSolver on the same line (dualnet/meta.go:20).  Off by default; with it off every
 * path launches the kernels it launches without this option.  State: one step counter t per trainer (uint64, starts at 0) and two flat
 * device buffers M1, M2 laid out like the learnables, zero at the start.  On every solver step (agz_trainer_apply, and the step inside
 * agz_trainer_batch / agz_train / agz_train_dev) the host increments t, computes rc1 = 1 / (1 - beta1^t) and rc2 = 1 / (1 - beta2^t) in
 * double and rounds each once to float; then per learnable element, in fp32, with the per-call lr and grad_scale:
 *     g1 = grad_scale * g
 *     g2 = g1 + l2reg * w                  (only if l2reg != 0)   } agz_solver_conf's l2reg / clip, as above
 *     g3 = min(max(g2, -clip), clip)       (only if clip > 0)     }
 *     m  = beta1 * m + (1 - beta1) * g3                           ((1 - beta1), (1 - beta2): rounded to float on the host)
 *     v  = beta2 * v + (1 - beta2) * (g3 * g3)
 *     w  = w + (-lr) * ((m * rc1) / (sqrtf(v * rc2) + eps))
 * With lr = 0 the moments move and w does not.  agz_trainer_batch steps the tower's gamma / beta and their moments inside the BatchNorm
 * backward kernel (no gradient is materialised, as for the other solvers) with the same t as the sweep that follows it in that step;
 * agz_trainer_eval touches neither t nor the moments.  The moments are 2 x the size of the learnables (2 x 7.7 GB at 19x19 / K = 256 /
 * 20 blocks / batch 256), allocated and zeroed when Adam is first turned on (AGZ_E_NOMEM if they do not fit; the settings are then
 * unchanged) and released, with t reset to 0, when it is turned off; a trainer that never asks for Adam allocates nothing.
 * agz_trainer_reset_solver also zeroes M1, M2 and t.  Sharded trainers: every rank makes the same call (a local call); a rank holds the
 * moment rows of the batch-shaped tensors it owns, the shared tensors' moments follow from the summed gradient identically on every rank —
 * no further collective.
 * set: AGZ_E_INVALID unless on is 0 or 1, 0 <= beta1 < 1, 0 <= beta2 < 1, eps > 0 and all are finite.  Adam and a momentum exclude each
 * other: set_adam with on = 1 while agz_solver_conf.momentum != 0, and agz_trainer_set_solver with momentum != 0 while Adam is on, return
 * AGZ_E_STATE and change nothing.  get: either pointer may be NULL; *step = t.
 * Tests: tests/test_adam_cpu.py (ABI, the restated definition against float64), tests/test_adam_gpu.py (off is untouched, recurrence,
 * fused = two-pass, headline width, oracle trajectory, checkpoint, validation, agz_train_dev), tests/test_adam_sharded_gpu.py. */
typedef struct agz_adam_conf { float beta1, beta2, eps; int32_t on; } agz_adam_conf; /* 16 bytes; defaults 0.9, 0.999, 1e-8, on = 0 */
int agz_trainer_set_adam(agz_trainer* t, const agz_adam_conf* conf);
int agz_trainer_get_adam(const agz_trainer* t, agz_adam_conf* out, uint64_t* step);
/* The two moments of learnable `index`: the indexing, shapes and — on a sharded trainer — row ownership of agz_trainer_get_velocity.
 * get: zeros while Adam is off.  set: AGZ_E_STATE while Adam is off.  Tests: test_adam_gpu.py (recurrence, checkpoint, validation),
 * test_adam_sharded_gpu.py. */
int agz_trainer_get_moments(const agz_trainer* t, int index, float* m, float* v, size_t n);
int agz_trainer_set_moments(agz_trainer* t, int index, const float* m, const float* v, size_t n);
/* Arithmetic of training's three GEMMs (forward convolution, data gradient, weight gradient): AGZ_COMPUTE_F32_MFMA (default),
 * AGZ_COMPUTE_BF16X3 (all three on the bf16 pipe; weights re-split on the device every step) or AGZ_COMPUTE_WINO_H2 (fp16x2
 * products throughout: forward = the DIRECT 3x3 convolution with fp16 hi/lo operands, weight image split on the device every step;
 * data gradient = the Winograd fp16x2 path with device-transformed weights; weight gradient = fp16 hi/lo operands split once per
 * layer; the first layer, 18 -> K, stays on BF16X3).  130 / 88 / 50 ms per step at 19x19, K = 256, 20 blocks, batch 256.  Every mode
 * meets the same gradient tolerance against the reference arithmetic — every gradient tensor within 2e-5 of its maximum, tested per
 * mode at the headline width (K = 256, 19x19) on several data draws — which is why the forward convolutions do NOT take the
 * Winograd path: its rounding (2e-6 of the output rms against 3e-7 for the direct forms) puts a pre-activation on the other side of
 * a ReLU than the reference on every other batch at that width. */
int agz_trainer_set_compute_mode(agz_trainer* t, int mode);
/* dual.Train(d, Xs, policies, values, batches, iterations) (dualnet/meta.go:16-54): lr 0.1 vanilla SGD, shuffleBatch
 * after every iteration (build RNG; Xs/policies/values are shuffled in place like the reference). */
int agz_train(agz_trainer* t, float* Xs, float* policies, float* values, int batches, int iterations, uint64_t seed,
              float* last_cost);
/* dual.Train over DEVICE tensors (e.g. agz_examples_tensors_dev): same loop and shuffleBatch stream as agz_train; the
 * shuffle permutes 4-byte row indices, batches are gathered device to device, the cost is read back once at the end.
 * The tensors themselves are left in place (the reference shuffles rows in place, meta.go:57-102; AZ.Learn discards
 * them right after, agogo.go:133). */
int agz_train_dev(agz_trainer* t, const float* Xs_dev, const float* policies_dev, const float* values_dev, int batches,
                  int iterations, uint64_t seed, float* last_cost);
/* Checkpoint of the trainable network in its full batch-shaped form (AZ.Save/AZ.Load agogo.go:175-209 for the side that
 * keeps learning; gob is Go-only, the format is specified in agogo_amd/csrc/ckpt.hpp, the one place that reads and writes it).
 * save: the file's form follows the trainer's state.  Without solver state "AGZTRN01" (l2reg / clip alone are the caller's
 * configuration, like lr, and are not stored); with a velocity (momentum != 0) "AGZTRN02": the 01 payload, agz_solver_conf, every tensor's
 * velocity; with Adam on "AGZTRN04": the 01 payload, agz_solver_conf, agz_adam_conf, uint64 t, every tensor's first and then second moment;
 * with running BatchNorm statistics (N > 0) "AGZTRN03": a uint32 inner form 1 / 2 / 3 (none / velocity / Adam), that body, then float
 * momentum, uint32 on, uint32 n_ops and per op {uint64 C, double N, double S_mean[C], double S_var[C]}.  A tied trainer
 * (agz_trainer_create_tied) writes "AGZTRN05": a uint32 inner form 1 .. 4 (the form a plain trainer in the same state would write), a
 * uint32 flags word (bit 0 = tied, always set; the other bits 0), then the body of that file after its magic, with the tied tensor sizes.
 * load: the file must match the configuration and the kind of the trainer (a tied file into a plain trainer and the reverse are refused,
 * also at BatchSize 1 where the tensor sizes coincide: that is what the flag is for).  A file without solver state zeroes the velocity (or the
 * moments and t) and keeps the options; one with a velocity sets the solver options and the velocity it carries and turns Adam off; an
 * Adam file sets the solver options, the Adam settings, t and the moments and turns Adam on.  A file with a BatchNorm block sets the tracking
 * setting and state it carries; any other resets the state to N = 0 and keeps the setting.
 * A bad file changes nothing, whatever its form: the WHOLE file — magic and form words, configuration, every count word, the options, the
 * BatchNorm block, and that it ends exactly where it should — is checked before the first value is applied; a truncated, overlong or
 * inconsistent file is AGZ_E_INVALID with the trainer untouched.  After a device error while the tensors are applied (AGZ_E_HIP) the
 * state is undefined.
 * Sharded: save is collective, rank 0 writes the plain trainer's file at the global batch; load is local, every rank reads its own rows.
 * Tests: tests/test_ckpt_cpu.py (the format and every refusal, without a GPU), tests/test_ckpt_golden_gpu.py (files written before the
 * codec existed), and the checkpoint tests of test_solver_gpu.py, test_adam_gpu.py, test_bn_tracking_gpu.py, test_tied_gpu.py. */
int agz_trainer_save(const agz_trainer* t, const char* path);
int agz_trainer_load(agz_trainer* t, const char* path);
/* dual.Infer's copy loop (dualnet/meta.go:141-146): row 0 of every learnable -> the inference net; commits it.  A trainer that holds
 * running BatchNorm statistics (N > 0, below) also hands them to the net (agz_net_set_bn_stats for every op) before the commit, whatever
 * the net's bn_mode; they matter under AGZ_BN_RUNNING.  Test: tests/test_bn_tracking_gpu.py (plays as trained). */
int agz_trainer_export(const agz_trainer* t, agz_net* net);
/* Running BatchNorm statistics (the reference asks gorgonia for them with momentum 0.997, dualnet/ermahagerdmonards.go:54; the update rule
 * is declared here, DESIGN §2 `bn-running`).  Per BatchNorm op — 2 * SharedLayers + 3 of them in the order of agz_net_set_bn_stats — and
 * channel c, in double on the device, on every training forward t while tracking is on:
 *     S_mean[c] = momentum * S_mean[c] + mu_t[c];   S_var[c] = momentum * S_var[c] + var_t[c];   N = momentum * N + 1
 *     estimates: mean[c] = (float)(S_mean[c] / N),  var[c] = (float)(S_var[c] / N)
 * mu_t / var_t: the batch mean and the biased batch variance (clamped at 0) that forward normalises with — the global batch's on a sharded
 * trainer — so after ONE forward the estimates are bit for bit what it normalised with, whatever the momentum.  S and N start at 0.  A
 * training forward is every forward of agz_trainer_forward_backward(_dev), agz_trainer_batch, agz_train(_dev),
 * agz_trainer_forward_backward_allreduce(_dev), on plain and sharded handles; after a call that fails part-way the state is undefined.
 * The accumulation runs inside the kernels that finalize the statistics: no launch and no synchronisation is added to the step, and with
 * tracking off every path launches exactly the kernels it launched before.  Turning tracking off keeps the state (export, eval and save
 * still use it), turning it on again continues it, another momentum changes only the coming updates.  Sharded: a local call, every rank
 * sets the same; every rank holds the same bits.
 * set_bn_tracking: AGZ_E_INVALID unless on is 0 / 1 and 0 <= momentum < 1, finite; the setting then stays as it was.  The default is
 * off, momentum 0.997.  get_bn_tracking: any pointer may be NULL; *weight = N.  Tests: tests/test_bn_tracking_cpu.py (ABI),
 * tests/test_bn_tracking_gpu.py (off is untouched, first step, float64 statistics, recurrence, validation), test_bn_tracking_sharded_gpu.py. */
int agz_trainer_set_bn_tracking(agz_trainer* t, int on, float momentum);
int agz_trainer_get_bn_tracking(const agz_trainer* t, int* on, float* momentum, double* weight);
/* 2 * SharedLayers + 3: Init, L1 / L2 of each shared layer (K channels each), the policy head (2), the value head (1) */
int agz_trainer_num_bn(const agz_trainer* t);
/* The estimates of op bn_index (C = its channel count).  get: AGZ_E_STATE while N == 0.  set: S = weight * value, N(op) = weight, weight > 0
 * (seeding a trainer from a net's statistics).  reset: S = 0, N = 0 for every op, the setting kept.
 * Tests: tests/test_bn_tracking_gpu.py (recurrence, validation, checkpoint). */
int agz_trainer_get_bn_stats(const agz_trainer* t, int bn_index, float* mean, float* var, size_t C);
int agz_trainer_set_bn_stats(agz_trainer* t, int bn_index, const float* mean, const float* var, size_t C, double weight);
int agz_trainer_reset_bn_stats(agz_trainer* t);
/* A held-out loss: the training graph's forward pass alone, every BatchNorm normalising with the estimates above instead of the batch's
 * statistics; *cost as agz_trainer_forward_backward.  No backward pass; learnables, gradients, velocity, S and N are untouched.  Needs
 * N > 0 for every op (AGZ_E_STATE otherwise); works with tracking on or off.  On a sharded handle the call is collective, only the cost
 * words are exchanged, and *cost is the global batch's, identical on every rank.  _dev: device buffers, cost may be NULL.
 * Tests: tests/test_bn_tracking_gpu.py (eval equals the forward it was made from, eval against float64), test_bn_tracking_sharded_gpu.py. */
int agz_trainer_eval(agz_trainer* t, const float* planes, const float* pi, const float* v, float* cost);
int agz_trainer_eval_dev(agz_trainer* t, const float* planes_dev, const float* pi_dev, const float* v_dev, float* cost);
/* The loss kind (DESIGN §2 `az-loss`).  AGZ_LOSS_REFERENCE, the default, is the reference's cost as restated by agz_trainer_forward_backward:
 * -mean(Pi z + (1 - Pi)(1 - z)) on the raw logits z and an MSE on the pre-tanh value output o (dualnet/dual.go:113-121).  The exported
 * net plays softmax(z) and tanh(o); AGZ_LOSS_ALPHAZERO trains exactly those.  With Bn the batch the loss is normalised by (BatchSize, or
 * the global batch of a sharded trainer), z [Bn][A] the logits, o [Bn] the value output, Pi / V the targets:
 *     per row b:  m_b = max_j z_bj    s_b = sum_j exp(z_bj - m_b)    lse_b = m_b + log s_b    p_bj = exp(z_bj - m_b) / s_b
 *                 S_b = sum_j Pi_bj   t_b = tanh(o_b)
 *     pcost = (1/Bn) sum_b ( S_b lse_b - sum_j Pi_bj z_bj )     ( = -sum Pi log softmax(z): a mean over the rows, NOT over rows x A )
 *     vcost = (1/Bn) sum_b (t_b - V_b)^2                          cost = pcost + vcost
 *     dz_bj = (S_b p_bj - Pi_bj) / Bn                             do_b = 2 (t_b - V_b)(1 - t_b^2) / Bn
 * The rows of Pi need not sum to 1: the factor S_b is part of the definition.  So is the subtraction of the row maximum before the
 * exponentials: logits of +-100 give finite costs and gradients.  The row reductions run in fp32 over one wave (ActionSpace <= 512:
 * AGZ_E_UNSUPPORTED above), the two cost sums in double in a fixed order: where every other reduction of a step runs in one workgroup, the
 * step reproduces to the bit, as the reference loss does there.
 * The kind is the caller's configuration, as the learn rate and agz_solver_conf are: NOT stored by agz_trainer_save (every AGZTRN0x format
 * is unchanged), and it covers every entry that runs a forward — agz_trainer_forward_backward(_dev), agz_trainer_batch, agz_train(_dev),
 * agz_train_replay(_sharded), the _allreduce forms, and agz_trainer_eval(_dev), which then returns a held-out cross-entropy — on plain,
 * tied, sharded and sharded-tied handles.  Sharded: a local call, every rank sets the same; the cost words travel in the exchange that
 * always carried them, no collective is added.  With the kind never set, or set back to AGZ_LOSS_REFERENCE, every path launches exactly
 * the kernels it launched before; the two small device buffers of the AlphaZero kind (dz [B][A], do [B]; 370 KB at B = 256, A = 362) are
 * allocated when it is first asked for.
 * set_loss: AGZ_E_INVALID for any other kind, the setting then stays as it was.
 * get_costs: the two terms of the last forward (training or eval) under either kind, *policy + *value being the cost that forward
 * returned; either pointer may be NULL; AGZ_E_STATE before the first forward.
 * Tests: tests/test_az_loss_cpu.py (ABI, the float64 module against the closed forms), tests/test_az_loss_gpu.py (off is untouched,
 * float64 parity at every shape, both head forms, stability, tied, reproducible, descent, eval, validation), test_az_loss_sharded_gpu.py. */
#define AGZ_LOSS_REFERENCE 0
#define AGZ_LOSS_ALPHAZERO 1
int agz_trainer_set_loss(agz_trainer* t, int kind);
int agz_trainer_get_loss(const agz_trainer* t, int* kind);
int agz_trainer_get_costs(agz_trainer* t, float* policy, float* value);

/* ---- batched self-play arenas: game.State + mcts.MCTS + agogo.Arena on device ---------------- */
#define AGZ_GAME_MNK 0  /* game/mnk  (m,n,k) */
#define AGZ_GAME_C4 1   /* game/c4   (rows=m, cols=n, k in a row) */
#define AGZ_GAME_KOMI 2 /* game/komi (m,n, capture-k) */
#define AGZ_GAME_WQ 3   /* game/wq   (m=n=size, komi) */
typedef struct agz_game_conf {
  int32_t kind;
  int32_t m, n, k;
  float komi;        /* wq: AdditionalScore (game/wq/game.go:181) */
  int32_t max_moves; /* arena safety cap on game length (the reference has no ko rule; 0 = 2*m*n) */
  int32_t encoder;   /* AGZ_ENC_* */
} agz_game_conf;
#define AGZ_ENC_TWOPLANE 0 /* cmd/tictactoe/main.go:26-47 : board(+-1, 0->0.001) + to-move plane, F=2 */
#define AGZ_ENC_WQ 1       /* WQEncoder, encoding_helper.go:29-68, F=18 */

/* mcts.Config (mcts/tree.go:15-29); Timeout is replaced by "exactly Budget simulations"  */
#define AGZ_DONT_PREFER_PASS 0
#define AGZ_PREFER_PASS 1
#define AGZ_DONT_RESIGN 2
typedef struct agz_mcts_conf {
  float PUCT;
  int32_t M, N;
  int32_t RandomCount;
  int32_t Budget;
  uint32_t RandomMinVisits;
  float RandomTemperature;
  int32_t DumbPass;
  float ResignPercentage;
  int32_t PassPreference;
} agz_mcts_conf;

/* Inferencer kinds an Agent can hold (mcts.Inferencer, mcts/mcts.go:15-18) */
#define AGZ_INF_NET 0    /* Agent.Infer over a dual net (agent.go:60-74) */
#define AGZ_INF_DUMMY 1  /* agogo.dummyInferer: uniform 1/ActionSpace policy, value +1 Black / -1 White agent (dummy.go:10-23) */
#define AGZ_INF_SCRIPT 2 /* mcts/example_test.go:40-72 dummyNN (tic-tac-toe script by move number) */
#define AGZ_INF_HASH 3   /* deterministic synthetic inferencer (integer hash of the position): parity tests */
#define AGZ_INF_UNIFORM 4 /* mcts/example_test.go:158-166 dummyNN2: 1/25 policy (len 25), value 1/25 */
#define AGZ_INF_CALLBACK 5 /* ANY mcts.Inferencer as a host function (agz_arena_set_inferencer_callback / agz_mcts_set_inferencer_callback) */

/* The `nn Inferencer` argument of mcts.New is an interface: Infer(state game.State) (policy []float32, value float32)
 * (mcts/mcts.go:15-18; tree.go:80).  A host inferencer meets the device search between its two kernels: after the descent every
 * expandable leaf of the agents that hold one is handed over as ONE batch — per leaf the encoder's input tensor (what Agent.Infer builds from
 * the state, agent.go:60-74), the board, the mover and MoveNumber() — and the callee fills one policy row and one value per leaf, exactly
 * what Infer returns: policy_len probabilities whose LAST entry is the pass probability (search.go:276), and the value as the
 * network reports it (the search itself turns it into `1 - value` for White, search.go:278-280).  The rows are consumed by the same
 * expansion kernel that reads a network's.  One host round trip per simulation step for all games of the arena: the boundary for
 * caller-supplied networks and a network-independent differential hook; AGZ_INF_NET keeps the whole step on the device.
 * Return 0; anything else aborts the search (AGZ_E_CALLBACK; reset the arena).  The function runs on the thread that called into libagz. */
typedef struct agz_leaf_batch {
  int32_t n;                  /* leaves in this call (>= 1) */
  int32_t features, height, width; /* geometry of `planes` (the arena's encoder) */
  int32_t policy_len;         /* floats per policy row (the value given at registration) */
  const float* planes;        /* [n][features][height][width] */
  const int32_t* board;       /* [n][height*width]  AGZ_NONE / AGZ_BLACK / AGZ_WHITE */
  const int32_t* to_move;     /* [n] the leaf state's ToMove() */
  const int32_t* move_number; /* [n] the leaf state's MoveNumber() */
  const int32_t* game;        /* [n] which game of the arena the leaf belongs to */
  float* policy;              /* OUT [n][policy_len] */
  float* value;               /* OUT [n] */
} agz_leaf_batch;
typedef int (*agz_infer_fn)(void* user, const agz_leaf_batch* batch);

/* MakeArena × n_games (arena.go:42-70): n_games independent games, each with agents A and B, each
 * agent with its own search tree (mcts.New, mcts/tree.go:80-103).  max_nodes = node-pool capacity per
 * tree; 0 = the default: FOUR searches' worth of expansions, 4 * (Budget + 2) * (ActionSpace + 1) nodes (at most 8 M) — a search adds at most
 * Budget + 1 expansions to the subtree kept from the one before, so a tree that keeps a fraction f of its nodes per move settles at
 * (Budget + 1)(ActionSpace + 1) / (1 - f): the default covers f <= 0.75.  A very NARROW tree keeps more and can outgrow it (the reference's
 * arena is unbounded up to MAXTREESIZE, search.go:23,78).  With max_nodes = 0 — the library chose the size — the pools therefore GROW when a
 * search could outgrow them (AGZ_POOL_GROW below is the default policy then: results unchanged, overflow impossible short of AGZ_E_NOMEM).  An
 * explicit max_nodes > 0 is the caller's memory budget (AGZ_POOL_STRICT): a tree whose pool fills stops growing for that move,
 * agz_arena_stats.tree_full counts it and agz_arena_play / agz_arena_selfplay return AGZ_E_TREE_FULL.  Examples: up to 2 * n_games * max_moves rows, at most 12 GiB per arena
 * (agz_arena_stats.examples_dropped counts rows that did not fit).  Budget 0 with several games: no simulations at all, every move
 * comes from prepareRoot (search.go:392-408). */
int agz_arena_create(agz_ctx* ctx, const agz_game_conf* game, const agz_mcts_conf* mcts, int n_games,
                     uint64_t seed, int max_nodes, agz_arena** out);
void agz_arena_destroy(agz_arena* arena);
/* Agent.NN / SwitchToInference / useDummy (agent.go:42-57,105-113): agent 0 = A, 1 = B. net may be NULL
 * for the non-NET kinds. */
int agz_arena_set_inferencer(agz_arena* arena, int agent, int kind, agz_net* net);
/* agent `agent` holds a host inferencer (AGZ_INF_CALLBACK, above).  policy_len >= the game's ActionSpace (<= 4096).  Setting another
 * kind with agz_arena_set_inferencer removes it. */
int agz_arena_set_inferencer_callback(agz_arena* arena, int agent, agz_infer_fn fn, void* user, int policy_len);
/* What a FULL node pool means (default: AGZ_POOL_GROW when the arena was created with max_nodes = 0, AGZ_POOL_STRICT with an explicit
 * max_nodes).  AGZ_POOL_STRICT: the tree stops growing, agz_arena_stats.tree_full counts it, and agz_arena_play /
 * agz_arena_selfplay / agz_mcts_search fail with AGZ_E_TREE_FULL — nothing is silently truncated, and every parity test runs this way.
 * AGZ_POOL_STOP_SEARCH: the reference's own rule — a tree at MAXTREESIZE stops being searched for that move and the game goes on
 * (search.go:23,78,229) — with max_nodes in MAXTREESIZE's place: the move is the best of the truncated search, the next move re-roots into
 * the free pool, tree_full still counts.  For long unattended self-play with a peaked network, where one narrow tree should not end the run. */
/* AGZ_POOL_GROW: pools that cannot overflow.  Before every search (agz_arena_begin_move; again inside agz_arena_simulate when a move runs more
 * simulations than its Budget) the host reads every tree's node count and, when the fullest tree could outgrow its pool — a search adds at
 * most (simulations + 1) x (ActionSpace + 1) nodes — re-allocates all pools at a larger capacity and copies the live trees over: node indices
 * and every result stay what they were (bit-exact against AGZ_POOL_STRICT with a large enough max_nodes).  One small read-back per move; a
 * re-allocation takes tens of milliseconds and is rare.  AGZ_E_NOMEM when the device cannot hold the larger pools.  A wall-clock search
 * (Budget <= 0) is covered slice by slice. */
#define AGZ_POOL_STRICT 0
#define AGZ_POOL_STOP_SEARCH 1
#define AGZ_POOL_GROW 2
int agz_arena_set_pool_policy(agz_arena* arena, int policy);
/* Start new games: fresh trees, empty boards, colour assignment.  a_is_black: per game 0/1, or NULL to
 * draw it from the arena RNG (arena.go:81-89 draws a.r.Intn(2)). */
int agz_arena_reset(agz_arena* arena, const uint8_t* a_is_black);
/* Arena.Play loop body for every unfinished game (arena.go:96-138): current agent Search
 * (mcts/search.go:92-164) -> record example -> Apply -> switch player -> Ended / two passes.
 * n_moves = how many plies to advance (<=0: until all games ended). */
int agz_arena_play(agz_arena* arena, int n_moves, int record);
/* Continuous self-play: like agz_arena_play, but a finished game is replaced at once by a fresh one (new trees,
 * colours drawn again) so all n_games slots stay busy; returns once n_games_target games have finished since the
 * last reset.  This is the `for e < episodes { ex = append(ex, a.SelfPlay()...) }` loop of AZ.Learn
 * (agogo.go:110-114) with the episodes running concurrently.  Needs both agents on one net (or synthetic). */
int agz_arena_selfplay(agz_arena* arena, int64_t n_games_target, int record);
/* Finer steps of one ply, for benchmarks and parity tests:
 *   begin_move   = updateRoot + prepareRoot (search.go:94-109)
 *   simulate(k)  = k x { pipeline (search.go:209-257) for every game, leaves coalesced into one
 *                  batched inference }
 *   end_move     = bestMove + Policies + Apply (search.go:151-161, arena.go:105-138) */
/* BUILD EXTENSION (no mcts.Config field): the simulations of one tree run in rounds of `lanes` (1..16) whose leaves are
 * evaluated as one batch — the deterministic, lane-ordered form of the reference's NumCPU goroutines sharing a tree with
 * the stored virtual loss (search.go:112-131, node.go:147-159,248-260; restated in oracle/mcts.hpp parallelRound, which
 * the device matches bit for bit).  For tournament latency: a single tree no longer evaluates one board at a time.
 * 1 (default) is the sequential search, the declared semantics of everything else in this library.  Changes the search
 * result (different, not worse, simulations); call between searches. */
int agz_arena_set_parallel(agz_arena* arena, int lanes);
/* BUILD EXTENSION (no mcts.Config field): leaf evaluation under a board symmetry, the AlphaGo Zero remedy for a network
 * that is not yet equivariant.  Square boards whose actions are their cells (mnk, komi, wq with m == n).
 * The eight maps: (R x)[i][j] = x[j][m-1-i] (RotateBoard), (T x)[i][j] = x[j][i]; S_k = R^(k&3) o T^(k>>2), k = 0..7, as an index map
 * (S_k x)[c] = x[src_k(c)]; inv(k): S_inv(k) o S_k = id; dst_k = src_inv(k).  S_0..S_3 are agz_examples_augment_rotate's images.
 * For a leaf of an agent holding AGZ_INF_NET the network's input is S_k of every plane of the encoder's tensor, the value is used as
 * returned, the prior of board cell c is policy_row[dst_k(c)], the pass prior policy_row[policy_len-1].  Every other inferencer kind is
 * unaffected (AGZ_INF_CALLBACK is handed the untransformed planes), and so are the recorded examples.
 *   AGZ_SYM_OFF        default: everything as without this call, bit for bit
 *   AGZ_SYM_RANDOM     k = mix32(ph ^ (uint32)seed ^ (uint32)(seed >> 32)) >> 29, ph = the position hash of AGZ_INF_HASH
 *                      (sum over cells of mix32(4 i + board[i] + 1), plus mix32(0xABCD0000 + to_move), uint32): a pure function of
 *                      (board, mover, seed) — independent of batch order, lanes, queues and the split step; agz_leaf_symmetry_of
 *   AGZ_SYM_FIXED + k  S_k at every leaf (tests, A/B runs)
 * AGZ_E_UNSUPPORTED for c4 or m != n, AGZ_E_STATE inside a move, AGZ_E_INVALID for any other mode.  Not stored in an arena checkpoint:
 * re-apply it after agz_arena_load and the continuation is bit for bit. */
#define AGZ_SYM_OFF 0
#define AGZ_SYM_RANDOM 1
#define AGZ_SYM_FIXED 8
int agz_arena_set_leaf_symmetry(agz_arena* arena, int mode, uint64_t seed);
/* The same definitions for a host inferencer (no context, no device).  agz_symmetry_map: src[c] = src_k(c) for the m*m cells
 * (1 <= m <= 19, 0 <= k < 8).  agz_symmetry_inverse: inv(k), or AGZ_E_INVALID.  agz_leaf_symmetry_of: AGZ_SYM_RANDOM's k of a position. */
int agz_symmetry_map(int m, int k, int32_t* src);
int agz_symmetry_inverse(int k);
int agz_leaf_symmetry_of(uint64_t seed, const int32_t* board, int cells, int to_move, int* k);
/* BUILD EXTENSION (no mcts.Config field; DESIGN.md §2 root-noise): Dirichlet noise mixed into the ROOT priors of every search, the
 * AlphaGo Zero exploration rule P(a) = (1 - eps) p(a) + eps eta(a), eta ~ Dir(alpha).  Opt-in, default off; off (or never called) is
 * everything as without this call, bit for bit: no launch, no allocation, no read-back.  While on, every path that runs prepareRoot
 * (agz_arena_begin_move, agz_arena_play, agz_arena_selfplay, agz_mcts_search) is followed by one launch that, per unfinished game and
 * for the tree of the agent that searches this move, rewrites the priors of the root's children — only those: noise never reaches
 * below a root.  Any inferencer kind, any game kind (c4 included), any lane count.
 * The definition (one copy, csrc/noise.hpp; IEEE double + - * /, integer and bit operations only — no libm — so host, device and a
 * restatement in any language with IEEE doubles agree bit for bit):
 *   RNG       SplitMix64: s += 0x9E3779B97F4A7C15; z = s; z = (z^(z>>30))*0xBF58476D1CE4E5B9; z = (z^(z>>27))*0x94D049BB133111EB; z ^= z>>31
 *   u01(z)    ((double)(z >> 12) + 0.5) * 2^-52
 *   ln_b(x)   x = m 2^e from the bits, m in [1,2); if m > 1.4142135623730951: m *= 0.5, e += 1; s = (m-1)/(m+1), s2 = s*s;
 *             acc = 0; for k = 12..0: acc = acc*s2 + 1.0/(2k+1); result e*0.6931471805599453 + (2.0*s)*acc
 *   exp_b(y)  y <= 0: 0.0 if y < -700; t = y*1.4426950408889634 + 0.5, k = floor(t), r = y - k*0.6931471805599453;
 *             acc = 1; for j = 16..1: acc = 1.0 + (acc*r)/j; result acc * 2^k
 *   key       one SplitMix64 output of the tree's own stream (the one randomizeChildren draws from: seeded per tree, re-seeded when a
 *             slot restarts, stored in arena checkpoints)
 *   gamma_i   child i = position i of the root's child block as it stands after prepareRoot; stream: SplitMix64 from state
 *             key + (i+1)*0xD1B54A32D192ED03.  Ahrens-Dieter GS (0 < alpha < 1): b = 1.0 + alpha/2.718281828459045; per round two
 *             outputs u1, u2, p = b*u1; p <= 1: x = exp_b(ln_b(p)/alpha), accept if u2 <= exp_b(-x); else x = -ln_b((b-p)/alpha), accept
 *             if u2 <= exp_b((alpha-1.0)*ln_b(x)); at most 64 rounds, then gamma_i = 0.  alpha == 1: gamma_i = -ln_b(u1), one output.
 *             alpha is the double obtained from the float passed in
 *   eta_i     (float)(gamma_i / S), S = gamma_0 + ... + gamma_{n-1} added in index order in double; S == 0: (float)(1.0/n)
 *   prior'    fadd(fmul(1.0f - eps, prior), fmul(eps, eta_i)) in float, one rounding per operation
 * A root without children gets nothing (no key is drawn; the observer reports n = 0).  A tree whose root already carries noise — a
 * second agz_mcts_search of the same position with no move between — keeps its priors and draws no second key; the mark is cleared
 * when a search gets a different root (re-rooted below the old one, or fresh).  Neither the setting nor the marks are stored in an arena
 * checkpoint (AGZARN01 unchanged; a loaded arena starts with every mark clear and no recorded draw): re-apply the setting after
 * agz_arena_load and the continuation is bit for bit.
 * AGZ_E_INVALID, with the setting unchanged, unless on is 0 or 1, 0 <= eps <= 1, 0 < alpha <= 1 (both finite) and reserved == 0;
 * AGZ_E_STATE inside a move. */
typedef struct agz_noise_conf { float eps, alpha; int32_t on, reserved; } agz_noise_conf;  /* 16 bytes; defaults 0.25, 0.3, on = 0 */
int agz_arena_set_root_noise(agz_arena* arena, const agz_noise_conf* conf);
int agz_arena_get_root_noise(agz_arena* arena, agz_noise_conf* out);
/* The last draw of `agent`'s tree in game g: its key and, per root child in the block order of that moment, the child's move and eta.
 * *n = the number of children (0: no draw yet; key is then 0); min(cap, *n) entries are copied (moves / eta may be NULL). */
int agz_arena_root_noise(agz_arena* arena, int g, int agent, uint64_t* key, int32_t* moves, float* eta, int cap, int* n);
/* The same definition without a context or a device: eta[0..n) of the draw `key`.  AGZ_E_INVALID unless 1 <= n <= 4096,
 * 0 < alpha <= 1 and eta != NULL. */
int agz_root_noise_of(uint64_t key, int n, float alpha, float* eta);
/* BUILD EXTENSION (DESIGN.md §2 visit-target): what an arena records as the POLICY ROW of an example.  Opt-in, default
 * AGZ_TARGET_REFERENCE; with it (or never called) everything is as without this call, bit for bit: the same launches, no allocation,
 * no read-back.
 *   AGZ_TARGET_REFERENCE  the reference's Policies (tree.go:128-142): normalised counts of the moves chosen at this board hash — in
 *                         practice a one-hot row of the move played; no row on a ply that chose Pass or Resign.
 *   AGZ_TARGET_VISITS     the root's visit distribution pi(a) ~ N(a)^(1/temperature), what AlphaZero trains on; one row on EVERY
 *                         searched ply whose root has a visited child, a ply that chose Pass or Resign included.
 * The kind changes the rows and how many are recorded, nothing else: the chosen move, the sort, the RNG draws, the trees, the games
 * and agz_mcts_policies (the cachedPolicies list) are the same.  Rows are ordinary example rows (agz_arena_get_examples, checkpoints,
 * the augmenters, the replay window and AGZ_LOSS_ALPHAZERO take any row).
 * The definition (one copy, csrc/target.hpp; IEEE double + - * /, integer and bit operations, ln_b / exp_b of the root noise above).
 * Children (move_i, N_i) of the root, N_i the uint32 visit count; A = the action space; tau = the double obtained from `temperature`:
 *   Nmax      max N_i; Nmax == 0: no target (no row; agz_visit_target_of returns AGZ_E_INVALID)
 *   w_i       64-bit integers.  tau == 1: N_i.  Otherwise 2^40 if N_i == Nmax, 0 if N_i == 0, else
 *             (uint64)(exp_b(ln_b((double)N_i / (double)Nmax) / tau) * 2^40), truncated
 *   S         the sum of the w_i, exact (below 2^53 for up to 4096 children): independent of the order of the children
 *   row[idx]  (float)((double)w_i / (double)S), idx = move_i for a board move, A for AGZ_PASS; every other of the A + 1 entries +0.0f
 * The setting is not stored in an arena checkpoint (AGZARN01 unchanged): re-apply it after agz_arena_load and the continuation is bit
 * for bit.  The single-tree agz_mcts_* handle records nothing and keeps AGZ_TARGET_REFERENCE.
 * AGZ_E_INVALID, with the setting unchanged, unless kind is 0 or 1, temperature is finite and > 0 and the reserved words are 0;
 * AGZ_E_STATE inside a move. */
#define AGZ_TARGET_REFERENCE 0
#define AGZ_TARGET_VISITS 1
typedef struct agz_target_conf { int32_t kind; float temperature; int32_t reserved[2]; } agz_target_conf;  /* 16 bytes; defaults 0, 1.0f */
int agz_arena_set_policy_target(agz_arena* arena, const agz_target_conf* conf);
int agz_arena_get_policy_target(agz_arena* arena, agz_target_conf* out);
/* The same definition without a context or a device: row[0 .. action_space] of n children.  AGZ_E_INVALID, with row untouched, for a
 * NULL pointer, n or action_space outside [1, 4096], a move that is neither in [0, action_space) nor AGZ_PASS, a move given twice, a
 * temperature that is not finite and > 0, and visits that are all 0. */
int agz_visit_target_of(const int32_t* moves, const uint32_t* visits, int n, int action_space, float temperature, float* row);
/* BUILD EXTENSION (no mcts.Config field; DESIGN.md §2 playout-cap): playout cap randomization, KataGo's remedy for self-play that pays
 * the whole Budget on every ply whether or not its row is worth training on.  Opt-in, default off; off (or never called) is everything
 * as without this call, bit for bit and launch for launch: no allocation, no read-back, no load in the step's kernels.  While on, every
 * ply of every game is, with probability p_full, a FULL search — mcts.Budget simulations, root noise (if that setting is on), a recorded
 * row (if the move records) — and otherwise a FAST search: fast_budget simulations, no root noise (no key is drawn), no row under either
 * policy-target kind.  Everything else of a ply is the same for both kinds: the move choice, randomizeChildren, cachedPolicies, Apply,
 * Ended, labelling and restart.
 * The definition (one copy, csrc/cap.hpp; integer and bit operations only):
 *   mix64     the SplitMix64 finaliser: z = (z^(z>>30))*0xBF58476D1CE4E5B9; z = (z^(z>>27))*0x94D049BB133111EB; z ^= z>>31
 *   z         mix64(seed ^ mix64(key + 0x9E3779B97F4A7C15 * (uint64)(ply + 1)))
 *   thr       (uint32)(p_full * 16777216.0f)       the product is exact; p_full = 1 gives 2^24 (always FULL), p_full = 0 gives 0 (always FAST)
 *   kind      AGZ_CAP_FULL if (uint32)(z >> 40) < thr, else AGZ_CAP_FAST
 *   budget    FULL: mcts.Budget      FAST: fast_budget
 * key is the game slot's own key (seeded at reset, advanced when the slot restarts in agz_arena_selfplay, stored in arena checkpoints)
 * and ply the number of moves of the game, both as they stand at agz_arena_begin_move; one small launch there makes the decisions.  No
 * RNG stream is consumed: the decision is a pure function of checkpointed state and the setting, so plies advanced from outside
 * (agz_arena_apply_moves, agz_arena_random_moves, agz_arena_set_state) need nothing — the next decision follows from the ply.
 * agz_arena_simulate(k) advances a per-move simulation index i; game g takes part in simulation i iff i < budget[g].  In a round of nl
 * lanes (agz_arena_set_parallel) that starts at index i0 game g runs clamp(budget[g] - i0, 0, nl) lanes; sims_total counts the
 * simulations actually run.  agz_arena_play and agz_arena_selfplay keep calling agz_arena_simulate(Budget), AGZ_POOL_GROW keeps sizing
 * for Budget.  While a round ends within fast_budget every game is active and the step is the one of an arena without the setting, the
 * split step included; so it is while every game of the arena is an unfinished FULL one.  Otherwise a round that reaches past
 * fast_budget is a tail step (a lane round may straddle fast_budget: the FAST games run the lanes it leaves them), and from
 * fast_budget on only the FULL games search: with none of them the remaining steps of the move are not enqueued at all; with one lane,
 * both agents on one shared net and a smaller batch that runs the whole batch's kernels (agz_net_min_same_batch) the FULL games are
 * packed to the front of the network batch, each board's result being the bit pattern the whole-arena batch gives; every other
 * configuration (lanes, two nets, callbacks, synthetic inferencers, no such smaller batch) runs those steps on the whole batch — the
 * same results and no time saved; where the arena would otherwise take the split step, slightly slower (a tail step is always the
 * joined step).  A game's search therefore never depends on what the other games drew.
 * Nothing is added to an arena checkpoint (AGZARN01 unchanged): re-apply the setting after agz_arena_load and the continuation is bit
 * for bit; until then searches are full searches.  The single-tree agz_mcts_* handle is not covered and keeps full searches.
 * AGZ_E_INVALID, with the setting unchanged, unless on is 0 or 1, 0 <= p_full <= 1 (finite), reserved == 0 and, when on is 1,
 * 1 <= fast_budget <= mcts.Budget; AGZ_E_UNSUPPORTED when on is 1 and mcts.Budget <= 0; AGZ_E_STATE inside a move. */
#define AGZ_CAP_FULL 0
#define AGZ_CAP_FAST 1
typedef struct agz_playout_cap_conf { float p_full; int32_t fast_budget; int32_t on; int32_t reserved; uint64_t seed; } agz_playout_cap_conf; /* 24 bytes; defaults 0.25, 0, 0, 0, 0 */
int agz_arena_set_playout_cap(agz_arena* arena, const agz_playout_cap_conf* conf);
int agz_arena_get_playout_cap(agz_arena* arena, agz_playout_cap_conf* out);
/* The decision of game g's current / last searched ply: the key and the ply it was made from, its kind and its budget (any pointer may
 * be NULL).  kind = -1 (key, ply, budget 0) before the game's first agz_arena_begin_move under the setting, after a reset and a load. */
int agz_arena_playout_cap(agz_arena* arena, int g, uint64_t* key, int32_t* ply, int32_t* kind, int32_t* budget);
/* Plies searched under each kind since the last reset / load (a small device buffer of its own: NOT in agz_arena_stats, NOT in a
 * checkpoint); either pointer may be NULL. */
int agz_arena_playout_cap_counts(agz_arena* arena, int64_t* full_plies, int64_t* fast_plies);
/* The same definition without a context or a device: the kind of ply `ply` of the slot with key `key`.  AGZ_E_INVALID unless ply >= 0,
 * 0 <= p_full <= 1 and kind != NULL. */
int agz_playout_cap_of(uint64_t seed, uint64_t key, int32_t ply, float p_full, int32_t* kind);
/* BUILD EXTENSION (no mcts.Config field; DESIGN.md §2 forced-playouts): KataGo's forced playouts and policy-target pruning at the root.
 * Opt-in, default off; off (or never called) is everything as without this call, bit for bit and launch for launch: no allocation, no
 * read-back, no load in the step's kernels (the setting rides on kernel arguments that leave one uniform branch not taken).
 * The definitions (one copy, csrc/forced.hpp; IEEE float and double operations rounded once, contraction off, integers).  For the
 * children i = 0..n-1 of a root as they stand in its child block:
 *   N_i, n_i   the stored visits (>= 1: a child is created with one visit) and the playouts n_i = N_i - 1
 *   B_i, P_i   the stored score sum and the stored prior (root noise, if on, is already in it)
 *   pv, T      the sum of N_i and the sum of n_i (= pv - n)
 *   q_i        Evaluate(B_i, N_i, player): B_i / N_i, and 1 - that for White, in float
 *   U(i, m)    fadd(q_i, fmul(fmul(PUCT, P_i), fdiv(sqrt((float)pv), fadd(1.0f, (float)m)))), the square root correctly rounded;
 *              U(i, N_i) is the value Node.Select maximises
 *   rhs_i      ((double)k * (double)P_i) * (double)T
 * Forced selection, at the root of every descent (below the root nothing changes): child i is forced iff n_i >= 1 and
 * (double)(n_i + mark_i) * (double)(n_i + mark_i) < rhs_i, mark_i being the child's stored virtual-loss mark in a lane round
 * (agz_arena_set_parallel) and 0 in the sequential search.  A forced child's value is +INFINITY, so Select's argmax and its tie rule
 * (the first maximum) pick the forced child with the lowest block index.  k = 0 forces nothing.  While the playout cap is on only FULL
 * plies force; a FAST ply searches as without this setting.
 * Pruned target, used when on, prune and AGZ_TARGET_VISITS all hold; only the recorded row changes (the move, the sort,
 * randomizeChildren, cachedPolicies and the trees are the same):
 *   c*         the child with the largest N_i, ties to the smallest move as an int (AGZ_PASS = -1 first);  U* = U(c*, N_c*)
 *   F_i        the largest integer f >= 0 with (double)f * (double)f <= rhs_i
 *   n'_i       c*: n_i.  n_i == 0: 0.  Otherwise N'_i = the smallest m in [N_i - min(F_i, n_i), N_i] with U(i, m) < U* (N_i if
 *              U(i, N_i) >= U*), with q_i, pv and U* held fixed; n'_i = N'_i - 1, and n'_i = 0 if N'_i < N_i and n'_i == 1 (a child
 *              reduced to a single playout is pruned outright)
 *   row        the AGZ_TARGET_VISITS definition applied to n' instead of N (weights from n'_i and max n' = n_c*, the temperature of
 *              agz_arena_set_policy_target); n_c* == 0: no row
 * With k = 0 the row is the playout-count target pi ~ (N - 1)^(1/tau): only the one visit every child is created with is removed.
 * With prune = 0 the row is the AGZ_TARGET_VISITS row of the forced search.  Under AGZ_TARGET_REFERENCE prune has no effect.
 * Nothing is added to an arena checkpoint (AGZARN01 unchanged): re-apply the setting after agz_arena_load and the continuation is bit
 * for bit.  The single-tree agz_mcts_* handle is not covered.
 * AGZ_E_INVALID, with the setting unchanged, unless on and prune are 0 or 1, k is finite with 0 <= k <= 64 and reserved == 0;
 * AGZ_E_STATE inside a move. */
typedef struct agz_forced_conf { float k; int32_t on; int32_t prune; int32_t reserved; } agz_forced_conf; /* 16 bytes; defaults 2.0f, 0, 1, 0 */
int agz_arena_set_forced_playouts(agz_arena* arena, const agz_forced_conf* conf);
int agz_arena_get_forced_playouts(agz_arena* arena, agz_forced_conf* out);
/* The same definitions without a context or a device.  agz_root_select_of: the block index Node.Select returns at a root with the forced
 * rule (*index; -1 if no value compares greater than -INFINITY) and whether that child was forced (*forced).  marks == NULL is the
 * sequential search (no mark, and no virtual-loss term); with marks White's view adds 3.0 to the score sum of a marked child, as a lane
 * round does.  k = 0 is plain Node.Select.  agz_pruned_target_of: the pruned playouts n' (pruned_playouts, [n], may be NULL) and the row
 * ([action_space + 1], Pass last) of a root.  Both refuse with AGZ_E_INVALID, leaving every output untouched: a NULL pointer (other than
 * marks / pruned_playouts), n outside [1, 4096], a player that is neither AGZ_BLACK nor AGZ_WHITE, puct outside (0, 1], k outside
 * [0, 64], a visit count of 0 and visits that sum past 2^32 - 1; agz_pruned_target_of also an action_space outside [1, 4096], a move that
 * is neither in [0, action_space) nor AGZ_PASS, a move given twice, a temperature that is not finite and > 0, and a root whose most
 * visited child has no playout (there is no row). */
int agz_root_select_of(const uint32_t* visits, const float* black_scores, const float* priors, const uint8_t* marks /* may be NULL */,
                       int n, int player, float puct, float k, int* index, int* forced);
int agz_pruned_target_of(const int32_t* moves, const uint32_t* visits, const float* black_scores, const float* priors, int n,
                         int action_space, int player, float puct, float k, float temperature,
                         uint32_t* pruned_playouts /* may be NULL, [n] */, float* row /* [action_space + 1] */);
int agz_arena_begin_move(agz_arena* arena);
int agz_arena_simulate(agz_arena* arena, int k);
int agz_arena_end_move(agz_arena* arena, int record);
/* Apply externally chosen moves instead of searching — moves[g] (a game.Single: cell / column, AGZ_PASS, AGZ_RESIGN) for
 * every game, ignored for finished games.  This is the opponent's reply in a tournament: the caller of Agent.Search
 * (agent.go:76-81) applies the opponent's move to its game.State and hands the new state to the next Search; here the
 * state lives on the device.  No example is recorded; the next search of either agent re-roots its tree by replaying
 * the moves played since its last search (updateRoot, search.go:424-500).  Every move must pass State.Check: a game
 * with an illegal move is left unchanged and AGZ_E_INVALID is returned (the other games are applied); AGZ_NO_MOVE
 * skips a game (e.g. to re-send a corrected move for one game only).  With two different nets the arena evaluates the
 * games in lockstep plies: keep all unfinished games at the same ply. */
#define AGZ_NO_MOVE (-32768)
int agz_arena_apply_moves(agz_arena* arena, const int32_t* moves);
/* BUILD EXTENSION — synthetic openings for benchmarks and parity tests ("for each slot play u uniformly-random
 * legal moves from the empty board"): game g plays n_moves[g] uniformly drawn legal board moves for alternating colours (Pass
 * only when the mover has no legal board move and the game has a pass), like agz_arena_apply_moves: no search, no example,
 * trees re-root at their next search.  Deterministic in (seed, g, moves played so far); restated by the oracle. */
int agz_arena_random_moves(agz_arena* arena, const int32_t* n_moves, uint64_t seed);

/* A game.State as the host holds it (game/state.go:125-156) — what mcts.SetGame / Agent.Search receive (tree.go:120-124,
 * agent.go:77-80) when the position was NOT reached by playing on the device. */
typedef struct agz_state {
  const int32_t* board;       /* [m*n] game.Colour per cell (State.Board()) */
  int32_t to_move;            /* State.ToMove() */
  int32_t n_moves;            /* moves applied so far = len(history) (State.MoveNumber(); c4 reports 1 regardless) */
  int32_t passes;             /* State.Passes(): consecutive passes so far (wq) */
  uint32_t hash;              /* State.Hash() for komi/wq (the running zobrist hash; mnk/c4 hash the board itself) */
  float captures_black, captures_white; /* komi: stones captured by each side (State.Score) */
  const int32_t* last_moves;  /* the most recent n_last_moves moves, oldest first (LastMove()/UndoLastMove() chain): tree reuse */
  int32_t n_last_moves;       /* replays them (search.go:424-469); with fewer than the plies since the previous Search a fresh root is built */
  const int32_t* historical;  /* [n_historical][m*n] boards after the last n_historical moves, oldest first (State.Historical): */
  int32_t n_historical;       /* WQEncoder's history planes (encoding_helper.go:29-68), at most 8 */
} agz_state;
/* overwrite game g of an arena with a host-side state (trees are kept: the next search re-roots or starts fresh) */
int agz_arena_set_state(agz_arena* arena, int g, const agz_state* st);

/* Checkpoint of a running arena: every game, both search trees of every game, every RNG state, the counters and the recorded examples, so
 * that self-play interrupted after a move continues EXACTLY as the uninterrupted arena would — bit for bit, trees and examples included
 * (the format is specified in agogo_amd/csrc/arena_ckpt.hpp, the one place that reads, writes and validates it).
 * save: only between moves; inside agz_arena_begin_move .. agz_arena_end_move it returns AGZ_E_STATE.  It enqueues on, and waits for, the
 * context's main queue, so an open split step is joined first.  It writes `path` + ".tmp" and renames that over `path` once every byte is
 * written and flushed: a crash during a save never destroys the previous checkpoint; on failure the temporary file is removed.  The arena
 * is never changed by a save.  Only the live prefix of every tree is written (20 bytes a node) plus 27.5 KB an example row at 19x19.
 * load: into an arena created with the same agz_game_conf, agz_mcts_conf and n_games; the file stores them and they are compared field by
 * field, a mismatch is AGZ_E_INVALID and agz_last_error() names the field (max_moves = 0 and its resolved value 2 * m * n are the same).  The
 * create-time seed need NOT match: every RNG state comes from the file.  The WHOLE file is validated before anything in the arena
 * changes — lengths, constants, configuration, and every index a kernel would follow (node counts, child blocks, moves, example links) — so a
 * truncated, overlong or inconsistent file is AGZ_E_INVALID with the arena exactly as it was, and never reaches a kernel.  After a device
 * error while the accepted file is applied (AGZ_E_HIP) the state is undefined.
 * NOT in the file, because they are the caller's configuration as lr is for a trainer: the inferencers (kind, net, callback), the lane
 * count (agz_arena_set_parallel), the pool policy, the split mode, timers and debug hooks.  The caller re-attaches them on the new arena
 * before or after the load; a bit-identical continuation needs the same ones (the same network parameters, the same lanes).
 * Capacity: node indices do not depend on the pool capacity, so a file loads into an arena of any max_nodes that holds its fullest tree.
 * An AGZ_POOL_GROW arena re-allocates its pools for the fullest tree plus the next search, as it does before every move
 * (agz_arena_pool_capacity, agz_debug.h, shows the growth); an AGZ_POOL_STRICT or AGZ_POOL_STOP_SEARCH arena whose pools are smaller than
 * the fullest tree fails with AGZ_E_NOMEM and stays unchanged, and so does any arena whose example buffer is smaller than the file's rows.
 * I/O failures (a path that cannot be opened, a failed write or rename) are AGZ_E_INVALID, as for agz_trainer_save / agz_trainer_load.
 * Not covered: the single-tree agz_mcts handle, the agz_examples store, a save inside a move.
 * Tests: tests/test_arena_ckpt_cpu.py (the format and every refusal, without a GPU), tests/test_arena_ckpt_gpu.py (continuations). */
int agz_arena_save(agz_arena* arena, const char* path);
int agz_arena_load(agz_arena* arena, const char* path);

/* --- observers (all copy into caller buffers) --- */
typedef struct agz_arena_stats {
  int64_t sims_total;    /* pipeline invocations (iter, search.go:181) */
  int64_t sims_nonnull;  /* playouts: non-null results (search.go:175-178) */
  int64_t nn_evals;      /* inferencer evaluations */
  int64_t moves_played;
  int64_t games_finished;
  int64_t examples;
  int32_t n_games;
  int32_t n_active;      /* games not yet ended */
  int32_t tree_full;     /* number of trees that overflowed their pool */
  int32_t examples_dropped; /* examples lost because the arena's example buffer was full (clear or append them earlier) */
  int64_t path_nodes;    /* measurement: nodes on the selected paths, summed over simulations (mean depth = / sims_total) */
  int64_t children_read; /* measurement: children Node.Select read, summed over simulations (12 B each, node.go:170-237) */
} agz_arena_stats;
int agz_arena_get_stats(agz_arena* arena, agz_arena_stats* out);
/* Agent statistics since the last reset (Agent.Wins / Loss / Draw, arena.go:156-171; Statistics, statistics.go):
 * A's wins = B's losses and vice versa.  AZ.Learn's gating rule is b_wins / (b_wins + a_wins) > UpdateThreshold
 * (agogo.go:155). */
int agz_arena_get_results(agz_arena* arena, int64_t* a_wins, int64_t* b_wins, int64_t* draws);
/* game state of game g: board [m*n] colours, to_move, move number, passes, ended, winner, a_is_black,
 * last best move */
typedef struct agz_game_state {
  int32_t to_move, move_number, passes, ended, winner, a_is_black, last_move, reserved;
  float score_black, score_white;
} agz_game_state;
int agz_arena_get_game(agz_arena* arena, int g, int32_t* board, agz_game_state* st);
/* moves played so far in game g (game.Single per ply); returns count via *n */
int agz_arena_get_history(agz_arena* arena, int g, int32_t* moves, int cap, int* n);
/* root children of agent's tree in game g after a search, in bestMove's fancySort order
 * (search.go:353): move, visits, blackScores, prior. Returns the number of children in *n. */
int agz_arena_root_children(agz_arena* arena, int g, int agent, int32_t* moves, uint32_t* visits,
                            float* black_scores, float* priors, int cap, int* n);
/* mcts.Nodes() analogue: nodes allocated in the tree pool */
int agz_arena_tree_nodes(agz_arena* arena, int g, int agent, int* n_nodes);
/* examples recorded so far (arena.go:105-123,146-155): planes [n, F*m*n], policy [n, A+1], value [n]
 * (labelled +1/-1/0 once the game has ended; before that the raw mover colour 1/2), game index [n].
 * Pass NULL buffers to query the count. */
int agz_arena_get_examples(agz_arena* arena, float* planes, float* policy, float* value, int32_t* game_idx,
                           int cap, int* n);
int agz_arena_clear_examples(agz_arena* arena);
/* Removes the examples of FINISHED games (labelled rows) from the arena's buffer and keeps the rows of games still in flight
 * (compacted, their per-game chains re-linked), so that continuous self-play can be harvested repeatedly without duplicates
 * and without losing the earlier plies of running games.  agz_examples_append_arena calls it (take semantics);
 * agz_arena_clear_examples, in contrast, discards everything — including the rows of running games. */
int agz_arena_drop_labelled_examples(agz_arena* arena);
/* device pointers of the example buffers (for an RCCL all-gather before dual.Train) */
int agz_arena_examples_dev(agz_arena* arena, float** planes, float** policy, float** value, int* n);
/* device flags [n]: 1 = the example's game has ended and Value is the +1/-1/0 label; 0 = still the raw mover colour */
int agz_arena_examples_labelled_dev(agz_arena* arena, const uint8_t** labelled);

/* ---- mcts.MCTS: ONE search tree on a caller-owned game.State (mcts/tree.go:80-142, mcts/search.go:92-164) ----------------
 * The drop-in for `mcts.New(game, conf, nn)` behind Agent.Search (agent.go:77-80): the host keeps its game.State, hands the
 * position over with agz_mcts_set_game and applies the returned move itself.  The tree persists between searches and is
 * re-rooted (updateRoot, search.go:424-500) when the new position follows from the previous one by agz_state.last_moves. */
typedef struct agz_mcts agz_mcts;
/* mcts.New (tree.go:80-103).  max_nodes: node-pool capacity (0 = default from Budget and the action space). */
int agz_mcts_create(agz_ctx* ctx, const agz_game_conf* game, const agz_mcts_conf* conf, uint64_t seed, int max_nodes, agz_mcts** out);
void agz_mcts_destroy(agz_mcts* mcts);
/* the `nn Inferencer` argument of mcts.New (mcts/mcts.go:15-18): AGZ_INF_* (net may be NULL for the synthetic kinds) */
int agz_mcts_set_inferencer(agz_mcts* mcts, int kind, agz_net* net);
/* mcts.New(game, conf, nn) with a caller-supplied Inferencer: `fn` is called once per simulation with the one leaf state (lane rounds:
 * up to `lanes` leaves) — the reference's own dummyNN (mcts/example_test.go:40-72) runs through this as it runs through mcts.New */
int agz_mcts_set_inferencer_callback(agz_mcts* mcts, agz_infer_fn fn, void* user, int policy_len);
/* AGZ_POOL_* for a single tree (see agz_arena_set_pool_policy) */
int agz_mcts_set_pool_policy(agz_mcts* mcts, int policy);
/* lanes per round (BUILD EXTENSION, see agz_arena_set_parallel) */
int agz_mcts_set_parallel(agz_mcts* mcts, int lanes);
/* leaf symmetry of a single tree (BUILD EXTENSION, see agz_arena_set_leaf_symmetry) */
int agz_mcts_set_leaf_symmetry(agz_mcts* mcts, int mode, uint64_t seed);
/* root noise of a single tree (BUILD EXTENSION, see agz_arena_set_root_noise); the observer reads THE tree's last draw */
int agz_mcts_set_root_noise(agz_mcts* mcts, const agz_noise_conf* conf);
int agz_mcts_root_noise(agz_mcts* mcts, uint64_t* key, int32_t* moves, float* eta, int cap, int* n);
/* (*MCTS).SetGame (tree.go:120-124) */
int agz_mcts_set_game(agz_mcts* mcts, const agz_state* st);
/* (*MCTS).Search(player) (search.go:92-164): SetToMove(player), updateRoot, prepareRoot, Budget simulations, bestMove,
 * prev = current.Clone(), cachedPolicies[{hash, best}]++.  The game is NOT advanced.  *best: cell / column, AGZ_PASS, AGZ_RESIGN. */
int agz_mcts_search(agz_mcts* mcts, int player, int32_t* best);
/* (*MCTS).Policies(current game) (tree.go:128-142): [ActionSpace+1] floats; NaN when no search of this position is cached */
int agz_mcts_policies(agz_mcts* mcts, float* policy, int cap);
/* root children after a search in bestMove's order (the debugging surface of (*MCTS).Children, unsafe_safe.go:15) */
int agz_mcts_root_children(agz_mcts* mcts, int32_t* moves, uint32_t* visits, float* black_scores, float* priors, int cap, int* n);
/* (*MCTS).Children(of) with the Node fields (*MCTS).Log / ToDot print (mcts/unsafe_safe.go:15, graph.go:34): the children of ANY
 * node of the live tree — node 0 is the root, child_ids feed further calls; *n = number of children (0: not expanded) */
int agz_mcts_children(agz_mcts* mcts, int node, int32_t* child_ids, int32_t* moves, uint32_t* visits, float* black_scores,
                      float* priors, int cap, int* n);
/* (*MCTS).ToDot() (mcts/graph.go:34-90): the live tree as Graphviz text — digraph "G", one HTML-table node per tree node with the
 * reference's rows (Node ID, Move, Player, Visits, Score = prior, State = the moves of its path on an empty board; "Value", the
 * evaluation a node was created with, is not kept on the device and prints as "-"), children in move order.  max_nodes > 0 limits
 * the output to the first max_nodes nodes of the pool (a top of the tree); *needed = bytes incl. the terminating 0 — call with
 * cap = 0 to size the buffer. */
int agz_mcts_to_dot(agz_mcts* mcts, int max_nodes, char* buf, size_t cap, size_t* needed);
/* mcts.Config.Timeout (mcts/tree.go:18,34) — the reference's OWN stopping rule: its Search runs simulations until the wall clock
 * says stop (search.go:132-133,196-197; Budget is inert there), 100 ms in mcts.DefaultConfig.  Opt-in: timeout_ms > 0
 * makes agz_mcts_search run simulations for that long (the clock is read between slices of device work; a Budget > 0 still caps the
 * search), timeout_ms = 0 (default) restores the deterministic "exactly Budget simulations".  NOT deterministic: the simulation count
 * depends on the machine — parity tests use Budget.  With Budget <= 0 (what the Go shim passes for a reference conf that only sets
 * Timeout) agz_mcts_create sizes the node pool for 65536 expansions when max_nodes is 0, and a pool that fills up ENDS the search
 * (AGZ_OK, the best move of the tree as it stands) instead of failing with AGZ_E_TREE_FULL: the reference's arena is unbounded and only
 * its clock stops it.  agz_mcts_last_simulations: simulations the last agz_mcts_search ran. */
int agz_mcts_set_timeout_ms(agz_mcts* mcts, int timeout_ms);
int agz_mcts_last_simulations(agz_mcts* mcts, int64_t* sims);
/* (*MCTS).Nodes() (tree.go:126): nodes of the live tree (the reference counts its arena slots, freed ones included) */
int agz_mcts_nodes(agz_mcts* mcts, int* n_nodes);
int agz_mcts_get_stats(agz_mcts* mcts, agz_arena_stats* out);
/* (*MCTS).Reset() (tree.go:249-276) completed to what Arena.Play does with it — Reset then a fresh mcts.New
 * (arena.go:140-141,175-176; the reference's Reset alone leaves an unusable tree): empty tree, empty policy cache */
int agz_mcts_reset(agz_mcts* mcts);

/* ---- example sets on device: what sits between AZ.SelfPlay and dual.Train ----------------------
 * []agogo.Example (datatypes.go:41-46) as three device arrays: Board [n, F*H*W], Policy [n, PolicyLen], Value [n].
 * The payload (27.4 KB per 19x19 example) never leaves HBM; the host handles 4-byte row indices only. */
typedef struct agz_examples agz_examples;
int agz_examples_create(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, agz_examples** out);
void agz_examples_destroy(agz_examples* ex);
int agz_examples_count(const agz_examples* ex, int64_t* n);
int agz_examples_clear(agz_examples* ex);
/* `ex = append(ex, a.SelfPlay()...)` (agogo.go:110-114) for all FINISHED games of a batched arena, in the reference's order:
 * game after game, each in ply order. Device-to-device.  The appended rows are TAKEN out of the arena
 * (agz_arena_drop_labelled_examples): calling it again appends only games that finished since. */
int agz_examples_append_arena(agz_examples* ex, agz_arena* arena);
/* append n rows from device buffers (e.g. the RCCL all-gathered examples of the other ranks) / host buffers */
int agz_examples_append_dev(agz_examples* ex, const float* planes_dev, const float* policy_dev, const float* value_dev, int64_t n);
int agz_examples_append_host(agz_examples* ex, const float* planes, const float* policy, const float* value, int64_t n);
/* device pointers of the raw store (rows in append order) — the send buffers of the RCCL all-gather */
int agz_examples_raw_dev(agz_examples* ex, float** planes, float** policy, float** value);
/* read back (tests / host-side consumers). *n = rows held; copies min(cap, *n) rows. */
int agz_examples_get(agz_examples* ex, float* planes, float* policy, float* value, int64_t cap, int64_t* n);
/* An Augmenter (datatypes.go:38-39; applied per recorded example, arena.go:115-120) built on RotateBoard
 * (encoding_helper.go:80-107): every example e is replaced by [e, rot e, rot^2 e, rot^3 e] — every plane of Board
 * and the m*n board part of Policy rotated, the pass entry and Value kept.  Non-square boards: AGZ_E_INVALID with
 * RotateBoard's message. */
int agz_examples_augment_rotate(agz_examples* ex);
/* BUILD EXTENSION: the dihedral Augmenter — every example e is replaced by [S_0 e .. S_7 e] (the eight maps of
 * agz_arena_set_leaf_symmetry; rows 0..3 of each group are agz_examples_augment_rotate's, bit for bit): planes and the board part
 * of Policy mapped, the pass entry and Value copied.  One pass over the store.  Same preconditions as agz_examples_augment_rotate. */
int agz_examples_augment_dihedral(agz_examples* ex);
/* `if maxExamples > 0 && len(ex) > maxExamples { shuffleExamples(ex); ex = ex[:maxExamples] }` (agogo.go:118-121;
 * maxExamples <= 0: skipped) followed by prepareExamples (agogo.go:211-249): shuffleExamples (agogo.go:251-257, build
 * RNG), batches = len/BatchSize, the first batches*BatchSize rows tensorised.  *batches may be 0 ("batches is nil",
 * agogo.go:123-125 — the caller's error). */
int agz_examples_prepare(agz_examples* ex, int BatchSize, int maxExamples, uint64_t seed, int* batches);
/* the prepared tensors: device pointers for agz_train_dev / host copies */
int agz_examples_tensors_dev(agz_examples* ex, float** Xs, float** Policies, float** Values, int64_t* rows, int* batches);
int agz_examples_get_tensors(agz_examples* ex, float* Xs, float* Policies, float* Values);
/* RotateBoard (encoding_helper.go:80-107) on `count` boards of m x n floats (host buffers; runs on the device). */
int agz_rotate_boards(agz_ctx* ctx, const float* boards, int count, int m, int n, float* out);
/* S_k (agz_arena_set_leaf_symmetry) on `count` boards of m x m floats (host buffers; runs on the device). k < 4: RotateBoard k times. */
int agz_symmetry_boards(agz_ctx* ctx, const float* boards, int count, int m, int k, float* out);

/* ---- replay window on device (BUILD EXTENSION, DESIGN.md §2 replay-window) --------------------------------------------------
 * The standard AlphaZero arrangement around dual.Train, which AZ.Learn (agogo.go:100-172) does not have: a sliding window over the most
 * recent `capacity` examples, minibatches drawn uniformly from it with replacement, each row under a random board symmetry applied as it
 * is drawn (nothing is materialised: agz_examples_augment_dihedral holds eight copies of every row).  Off unless used; agz_examples_* and
 * agz_train_dev are untouched by it.
 * Storage: a ring of `capacity` rows in the row format of agz_examples (planes [F*H*W], policy [PolicyLen], value; fp32), three device
 * arrays allocated once at create.  total = rows ever appended, live = min(total, capacity); logical row j (0 = the oldest live row) sits in
 * slot (total - live + j) mod capacity; an append writes slot total mod capacity, then total++.
 * The draw (agogo_amd/csrc/replay.hpp, one host/device definition): out(seed, i) = the i-th output (from 0) of the build's SplitMix64
 * seeded with `seed`.  Row r of minibatch `step` (every minibatch `rows` rows) is draw q = step * rows + r (uint64) and uses z0 =
 * out(seed, 2q), z1 = out(seed, 2q + 1): j = (z0 * live) >> 64 (128-bit product), k = z1 >> 61 if symmetric else 0.  A whole run is one
 * sequential SplitMix64 stream, two outputs per row; symmetric on or off draws the same rows.
 * Tests: tests/test_replay_cpu.py, tests/test_replay_gpu.py, tests/test_replay_learn_gpu.py. */
typedef struct agz_replay agz_replay;
/* capacity < 1 or a bad shape: AGZ_E_INVALID.  The device cannot hold the ring: AGZ_E_NOMEM, nothing stays allocated. */
int agz_replay_create(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity, agz_replay** out);
/* The same window with its planes kept as 2-bit codes (DESIGN.md §2 replay-packed; the layout is agogo_amd/csrc/replay_pack.hpp's, one
 * host/device definition).  The planes are 95 % of a row and an encoder writes only four bit patterns into them, so a 19x19 / 18-plane row
 * falls from 27 444 to 3 108 bytes, losslessly.  `palette` holds n_palette (1..4) floats taken as 32-bit PATTERNS and compared as uint32,
 * never as floats: +0.0 and -0.0 are different entries, a NaN pattern is a legal one; two equal patterns or an n_palette outside 1..4 are
 * AGZ_E_INVALID, as is everything agz_replay_create refuses (AGZ_E_NOMEM likewise).  A cell's code is the index of its pattern in the
 * palette; 16 codes to a uint32, wpp = (H*W + 15) / 16 words per plane, every plane starts a word: cell c of plane f of a row is bits
 * [2 * (c & 15), +2) of word f * wpp + (c >> 4), unused high bits zero.  Storage: packed [capacity][F * wpp] uint32, policy and value fp32
 * as before.  The handle is an agz_replay: every agz_replay_* call and agz_train_replay work on it with the meaning documented here, get
 * and the samplers give back the palette entries' bits exactly (the sampler decodes as it draws, k_replay_sample_packed).
 * APPENDS to a packed window take ALL ROWS OR NONE: every row handed in is checked against the palette first, including the rows an
 * append longer than the capacity would skip.  A cell outside the palette: AGZ_E_INVALID, the message names the first bad row, element
 * and bit pattern (the smallest linear index), and the window is unchanged — total, live and every stored bit.  The check costs one
 * small read-back, so A PACKED APPEND SYNCHRONISES THE CONTEXT'S QUEUE ONCE (append_dev included); an append happens once per epoch.
 * Tests: tests/test_replay_pack_cpu.py, tests/test_replay_packed_gpu.py, tests/test_replay_packed_learn_gpu.py. */
int agz_replay_create_packed(agz_ctx* ctx, int Features, int Height, int Width, int PolicyLen, int64_t capacity, const float* palette,
                             int n_palette, agz_replay** out);
/* The four patterns an encoder's planes hold (host only, no context): AGZ_ENC_WQ {+0.0f, -0.0f, 1.0f, -1.0f} (the opponent's empty cells
 * are -0.0), AGZ_ENC_TWOPLANE {0.001f, 0.0f, 1.0f, -1.0f}; *n = 4.  An unknown encoder: AGZ_E_INVALID. */
int agz_encoder_palette(int encoder, float palette[4], int* n);
/* The packing without a context or a device: n rows of Features planes of `cells` floats into n * Features * ((cells + 15) / 16) words.
 * `words` may be NULL (validate only); first_bad (may be NULL) receives the smallest linear element index row * Features * cells + e
 * whose pattern is not in the palette, or -1.  A bad cell: AGZ_E_INVALID, `words` untouched.  A bad palette: AGZ_E_INVALID. */
int agz_replay_pack_host(const float* planes, int64_t n, int Features, int cells, const float* palette, int n_palette, uint32_t* words,
                         int64_t* first_bad);
/* What a window holds on the device, either kind: *packed = 1 for agz_replay_create_packed's, row_bytes = the bytes of one row as stored
 * (planes or words, policy, value), device_bytes = capacity * row_bytes, the three arrays of create.  Any of the three may be NULL. */
int agz_replay_storage(const agz_replay* rp, int32_t* packed, int64_t* row_bytes, int64_t* device_bytes);
void agz_replay_destroy(agz_replay* rp);
/* any of the three may be NULL */
int agz_replay_count(const agz_replay* rp, int64_t* live, uint64_t* total, int64_t* capacity);
/* empties the window (total = 0); the storage stays */
int agz_replay_clear(agz_replay* rp);
/* Appends.  n rows are n single-row appends in order: with n > capacity only the last `capacity` rows survive (total still grows by n).
 * append_examples: the raw store of `ex` in append order, device to device on the context's queue; `ex` is unchanged and must live on the
 * window's context with the window's shape (AGZ_E_INVALID otherwise).  append_dev: device buffers, asynchronous.  append_host: host
 * buffers, returns when they have been read. */
int agz_replay_append_examples(agz_replay* rp, agz_examples* ex);
int agz_replay_append_dev(agz_replay* rp, const float* planes_dev, const float* policy_dev, const float* value_dev, int64_t n);
int agz_replay_append_host(agz_replay* rp, const float* planes, const float* policy, const float* value, int64_t n);
/* read back logical rows [j0, j0 + cnt), oldest first (tests / host-side consumers); any buffer may be NULL.  AGZ_E_INVALID unless
 * 0 <= j0, 0 <= cnt, j0 + cnt <= live. */
int agz_replay_get(agz_replay* rp, int64_t j0, int64_t cnt, float* planes, float* policy, float* value);
/* Minibatch `step` of `rows` rows, ONE kernel launch that computes (j, k) of every row itself — no index array, no synchronisation:
 * X [rows, F, H, W] = S_k of the planes of window row j, Pi [rows, PolicyLen] = S_k of its policy's board part with the pass entry (and
 * anything after it) copied, V [rows] = its value; S_k as in agz_symmetry_map.  sample_dev: device buffers, asynchronous on the context's
 * queue.  sample: host buffers.  rows < 1: AGZ_E_INVALID.  symmetric != 0 needs Height == Width and PolicyLen >= Height * Width
 * (AGZ_E_INVALID with agz_examples_augment_rotate's messages).  An empty window: AGZ_E_STATE. */
int agz_replay_sample_dev(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X_dev, float* Pi_dev, float* V_dev);
int agz_replay_sample(agz_replay* rp, int rows, uint64_t seed, uint64_t step, int symmetric, float* X, float* Pi, float* V);
/* rows [row0, row0 + cnt) of minibatch `step` of `rows` rows: out row r = row (row0 + r) of what agz_replay_sample_dev(rows) gives, bit for
 * bit; the buffers hold cnt rows.  The same kernel and ONE launch; with row0 = 0 and cnt = rows it is agz_replay_sample_dev.  What rank
 * rho of a sharded trainer draws of the global minibatch (agz_train_replay_sharded): rows = n_ranks * B, row0 = rho * B, cnt = B.
 * AGZ_E_INVALID unless rows >= 1, row0 >= 0, cnt >= 1 and row0 + cnt <= rows; the symmetric preconditions and the empty window as above. */
int agz_replay_sample_slice_dev(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric,
                                float* X_dev, float* Pi_dev, float* V_dev);
int agz_replay_sample_slice(agz_replay* rp, int rows, int row0, int cnt, uint64_t seed, uint64_t step, int symmetric,
                            float* X, float* Pi, float* V);
/* The digest of a window's LOGICAL content (agogo_amd/csrc/replay.hpp, one host/device definition; DESIGN.md §2 replay-sharded): with
 * mix64 the SplitMix64 finaliser, rowlen = F*H*W + PolicyLen + 1 and bits(j, e) the 32-bit pattern of element e (planes, then policy, then
 * value) of logical row j (0 = the oldest live row; a packed window's decoded palette pattern),
 *     digest = live + sum over j < live, e < rowlen of mix64(mix64(j * rowlen + e) ^ bits(j, e))          (uint64, wrapping)
 * An integer sum: the same whatever the launch geometry, for a packed and an unpacked window fed the same rows, and wherever the ring
 * sits physically.  Patterns, not floats: +0.0 and -0.0 differ.  agz_replay_digest reads the window once on the device and SYNCHRONISES
 * THE CONTEXT'S QUEUE ONCE; agz_replay_digest_host is the same definition over n rows in host arrays (planes [n][Features * cells],
 * policy [n][PolicyLen], value [n]) and needs no context: digest_host of agz_replay_get(0, live) is agz_replay_digest.  Replicas of a
 * window (one per rank) hold the same rows exactly if their digests agree, up to a 2^-64 collision. */
int agz_replay_digest(agz_replay* rp, uint64_t* digest);
int agz_replay_digest_host(const float* planes, const float* policy, const float* value, int64_t n, int Features, int cells, int PolicyLen,
                           uint64_t* digest);
/* The same draw without a context or a device: j[r] in [0, n) and k[r] for the `rows` rows of minibatch `step` over n live rows (either
 * array may be NULL, not both).  AGZ_E_INVALID unless rows >= 1 and n >= 1. */
int agz_replay_draw(uint64_t seed, uint64_t step, int rows, int64_t n, int symmetric, int64_t* j, int32_t* k);
/* dual.Train's loop over sampled minibatches: for step = 0 .. steps - 1, minibatch `step` of BatchSize rows is sampled straight into the
 * trainer's batch buffers and the trainer takes exactly the step agz_train_dev takes per batch (learn rate 0.1, the solver options / Adam
 * that are set).  live is read once at entry; no host synchronisation between steps; the cost of the last step is read back at the end
 * (last_cost may be NULL; 0 when steps == 0).  The trainer and the window must share a context and a shape (AGZ_E_INVALID); an empty
 * window is AGZ_E_STATE; a SHARDED trainer (agz_trainer_create_sharded / _sharded_tied) is AGZ_E_UNSUPPORTED: its route is the
 * collective agz_train_replay_sharded. */
int agz_train_replay(agz_trainer* t, agz_replay* rp, int steps, uint64_t seed, int symmetric, float* last_cost);
/* agz_train_replay on a SHARDED trainer (agz_trainer_create_sharded / _sharded_tied; DESIGN.md §2 replay-sharded, §7).  COLLECTIVE: every
 * rank calls it with its own handle and its own REPLICA of the window (the same rows in the same logical order, e.g. every rank appending
 * what agz_examples_allgather gave it), and with the same steps, seed, symmetric and verify.  Declared result: what agz_train_replay
 * computes on the single-process trainer of the same kind at the GLOBAL BatchSize — step s trains on minibatch s of n_ranks * B rows of
 * the window, of which this rank draws rows [row0, row0 + B) itself (row0: agz_trainer_shard; agz_replay_sample_slice_dev), with the
 * differences §7 declares for every sharded step and no other.  No collective is added to a step and nothing is exchanged for the draw.
 * Entry, before anything is trained: the local checks of agz_train_replay, agreed on by all ranks (a failing rank returns its error, the
 * others AGZ_E_PEER), then ONE all-gather of {total, capacity, live, packed flag, digest}, digest = agz_replay_digest if verify != 0,
 * else 0.  If any rank's tuple differs from rank 0's, EVERY rank returns AGZ_E_STATE, the message names the first differing rank and
 * field, and no parameter changed.  verify = 0 checks the counts only: replicas with equal counts and different rows then train on
 * different data without an error.  A handle that is not sharded: AGZ_E_STATE (use agz_train_replay).  A rank whose sampler launch fails
 * in a step still enters that step's collectives; the error ends the run on every rank, as in agz_train_dev. */
int agz_train_replay_sharded(agz_trainer* t, agz_replay* rp, int steps, uint64_t seed, int symmetric, int verify, float* last_cost);
/* Checkpoint of a window (DESIGN.md §2 replay-ckpt): the live rows in LOGICAL order, oldest first, with total, the saving capacity, the
 * form (fp32 planes or 2-bit codes with their palette) and agz_replay_digest of the window, so that a run interrupted between two epochs
 * continues EXACTLY as the uninterrupted one — the same slots, samples, digests and trained parameters, bit for bit (the format is
 * specified in agogo_amd/csrc/replay_ckpt.hpp, the one place that reads, writes and validates the header and the lengths).
 * save: joins the context's queue (every append enqueued so far is in the file), writes `path` + ".tmp", flushes and fsyncs it and renames
 * it over `path`: a crash during a save never destroys the previous checkpoint; on failure the temporary file is removed.  The window is
 * never changed by a save.  An empty window is a valid file, and so is a window that a load into a larger capacity left not yet full: its
 * file carries its live count in the (informational) capacity word, so that the file's own rule live == min(total, capacity) holds.  A packed window writes its words as they are (8.8 times fewer bytes at 19x19).
 * load: replaces the window's content.  total := the file's total, live := min(the file's live, capacity), and the live rows are the NEWEST
 * live rows of the file, each in the slot replay.hpp's arithmetic gives the append that wrote it: into a window of the saving capacity every
 * row sits where it sat and later appends go where they would have gone; into a smaller window only the newest rows survive, as after one
 * long append; into a larger one the window is simply not yet full.  Features, Height, Width and PolicyLen must match (AGZ_E_INVALID,
 * agz_last_error() names the field).  The form need NOT match, the chunks are converted on the device as they arrive: an fp32 file into a
 * packed window looks every cell up in the window's palette, a packed file into an fp32 window decodes with the file's palette, a packed
 * file into a packed window of another palette order remaps the codes through the patterns (every palette entry of the file must be in
 * the window's palette, else AGZ_E_INVALID).
 * A BAD FILE CHANGES NOTHING.  A window does not fit in host memory twice, so the file is read twice: the first pass streams every chunk
 * into a device staging buffer, where one kernel adds up the digest and checks what a later kernel would trust, and the ring is not
 * touched; only when the whole file has passed does the second pass stream it into the ring.  AGZ_E_INVALID with total, live and every
 * stored bit as they were: a missing file, bad magic or end mark, a truncated or overlong file, live != min(total, capacity), live >
 * total, bad form or palette words, another shape, a code of a packed file that is not below its n_palette, a set bit past the last cell
 * of a plane's last word, a cell of an fp32 file that is not in a packed window's palette (the message names the first such row,
 * element and pattern), and rows whose digest is not the header's.  After a device error in the second pass (AGZ_E_HIP) the content is
 * undefined.  I/O failures are AGZ_E_INVALID, as for agz_trainer_save and agz_arena_save.  The host holds two page-locked staging
 * buffers (256 MB each at most), never the window.
 * Sharded use is not a call of its own: every rank loads the same file into its replica, the digests agree and
 * agz_train_replay_sharded(verify = 1) accepts them.
 * NOT in the file: the window's capacity as a requirement (any capacity loads), the sampler's seed and step (the caller's arguments).
 * Not covered: the agz_examples store, the arena's example buffer (agz_arena_save holds it), compression beyond the packed form,
 * asynchronous or incremental saves, a save while agz_train_replay runs on another thread.
 * Tests: tests/test_replay_ckpt_cpu.py (the format and every header refusal, without a GPU), tests/test_replay_ckpt_gpu.py (round trips,
 * continuations, conversions, refusals), tests/test_replay_ckpt_learn_gpu.py (AZ::Learn resumed at an epoch boundary). */
int agz_replay_save(agz_replay* rp, const char* path);
int agz_replay_load(agz_replay* rp, const char* path);

/* ---- multi-GPU exchange over RCCL / xGMI -------------------------------------------------------------------
 * Self-play games shard across GPUs with NO data-path collective (one agz_ctx + arena set per GPU).  The path has exactly
 * two exchange steps, both around dual.Train: the union of all ranks' examples (agogo.go:110-133: `ex` holds every episode
 * before shuffleExamples / prepareExamples) and the gradient sum of the data-parallel training step (dualnet/meta.go:33-40).
 * librccl is loaded on first use; without it these calls fail with AGZ_E_UNSUPPORTED (no single-GPU fallback). */
typedef struct agz_comm agz_comm;
#define AGZ_COMM_ID_BYTES 128
/* one process driving n GPUs (a Go host: one goroutine locked to an OS thread per ctx): ncclCommInitAll over the ctxs' devices;
 * comms[i] belongs to ctxs[i].  Collective calls on the n communicators must be issued concurrently, one thread per ctx. */
int agz_comm_init_all(agz_ctx* const* ctxs, int n, agz_comm** comms);
/* one process per GPU: rank 0 makes the id (agz_comm_unique_id), the host ships its AGZ_COMM_ID_BYTES bytes to the other ranks */
int agz_comm_unique_id(void* id128);
int agz_comm_init_rank(agz_ctx* ctx, int n_ranks, int rank, const void* id128, agz_comm** out);
void agz_comm_destroy(agz_comm* comm);
int agz_comm_rank(const agz_comm* comm);
int agz_comm_size(const agz_comm* comm);
/* every rank's example set becomes the union of all ranks' sets, in rank order (each rank's rows keep their order) */
int agz_examples_allgather(agz_comm* comm, agz_examples* ex);
/* sum the flat gradient buffer of the trainer over all ranks (one collective per step, in place, asynchronous on the ctx
 * stream); follow with agz_trainer_apply(t, lr, 1.0f / agz_comm_size(comm)) */
int agz_trainer_allreduce(agz_comm* comm, agz_trainer* t);
/* The data-parallel step with the reduction UNDER the backward pass: agz_trainer_forward_backward (host buffers) /
 * agz_trainer_forward_backward_dev (device buffers) on this rank's batch, every slice of the flat gradient buffer — the heads, then
 * layer L .. 0 as the backward pass finishes them — summed over the ranks on the communicator's own queue while the rest of the
 * backward runs (the G19 trainer's buffer is 7.7 GB: as one call after the backward it would cost about as much xGMI time as the
 * whole compute step).  On return (asynchronous on the ctx stream, like agz_trainer_allreduce) the gradients are the sums; the result
 * equals forward_backward + agz_trainer_allreduce.  Follow with agz_trainer_apply(t, lr, 1.0f / agz_comm_size(comm)).  Every rank
 * must call it for the same step (the slices are collectives, issued in the same order everywhere).  Errors: a rank that fails part-way
 * still enters every collective of the step, and the step ends with a one-word status exchange — the call then fails on EVERY rank
 * (AGZ_E_PEER on the ranks that were fine themselves) and the gradients must not be applied; an error of RCCL itself is fatal for the
 * process group (destroy the communicator).  dualnet/meta.go:16-54. */
int agz_trainer_forward_backward_allreduce(agz_comm* comm, agz_trainer* t, const float* planes, const float* pi, const float* v, float* cost);
int agz_trainer_forward_backward_allreduce_dev(agz_comm* comm, agz_trainer* t, const float* planes_dev, const float* pi_dev, const float* v_dev, float* cost);
/* Sharded training: dual.Train (dualnet/meta.go:16-54) at the GLOBAL batch conf->BatchSize, split over the ranks of the communicator.
 * The reference's BatchNorm gamma / beta [BatchSize,C,H,W] and FC biases [BatchSize,units] (dualnet/dual.go:105-132) give every batch row
 * its own parameters: rank r of n owns rows [r*B, (r+1)*B), B = BatchSize / n, and holds only those rows of them (and of their gradients).
 * The shared tensors (filters, the heads' 1x1 convolutions, the FC weights) are replicated and their gradients summed over the ranks;
 * BatchNorm takes its statistics over all BatchSize rows (the ranks' partial sums are gathered and summed in rank order: the same bits on
 * every rank) and the loss is normalised by the global batch.  The result is dual.Train at BatchSize, not an average of n smaller runs.
 * BatchSize must be a multiple of agz_comm_size(comm) (else AGZ_E_INVALID); the trainer lives on the communicator's ctx, which must
 * outlive it together with the communicator.  On such a handle:
 *   forward_backward(_dev), batch, train, train_dev, export, save are COLLECTIVE: every rank calls them for the same step, in the same
 *     order.  planes / pi / v of forward_backward and batch are this rank's B rows; *cost is the GLOBAL cost, bit-identical on every
 *     rank; the shared tensors' gradients come back summed.  train / train_dev take the GLOBAL tensors (the same on every rank, e.g.
 *     agz_examples_tensors_dev after agz_examples_allgather and agz_examples_prepare with the global BatchSize and a shared seed) and the
 *     single-process shuffle stream; each rank trains its rows of every global batch.  export gives every rank's net rank 0's row 0
 *     (broadcast); save has rank 0 write the file of a plain trainer with the global conf (gathered tensor by tensor).
 *   apply, init_random, load, param_info / get_param / set_param / get_grad are local: batch-shaped tensors are this rank's row slice
 *     (n_elems reports the slice), shared tensors are whole; apply takes no 1/n (the loss is already the global batch's); init_random(seed)
 *     draws exactly those rows of a plain trainer's init_random(seed) at the global batch; load reads a global checkpoint's rows.
 *   agz_trainer_allreduce and agz_trainer_forward_backward_allreduce(_dev) return AGZ_E_STATE.
 * Errors of a collective call: a rank that fails part-way still enters every remaining collective and all ranks exchange a status word —
 * the call fails on EVERY rank (AGZ_E_PEER on the ranks that were fine), nobody hangs, and the next call is an ordinary one.  After a
 * failed step the learnables are undefined (see agz_trainer_batch). */
int agz_trainer_create_sharded(agz_comm* comm, const agz_net_conf* conf, agz_trainer** out);
/* Tied sharded training (DESIGN §2 `tied-affine`, §7): the handle computes what agz_trainer_create_tied computes at BatchSize = n * B, over the n
 * ranks of the communicator, each holding B = BatchSize / n rows of the step and EVERY tied tensor whole.
 *   Forward, cost and BatchNorm statistics are those of the agz_trainer_create_sharded handle whose batch-shaped tensors hold the tied tensor
 *     in every row — for the same n bit for bit.
 *   The gradient of a tied tensor is built from one double partial per rank.  Each rank forms its partial over its own B rows exactly as the
 *     tied trainer does: fp32 per-row terms accumulated in double, four interleaved row slices added in slice order (the head tensors: the
 *     rows in row order), NOT rounded.  The n partials are added in rank order in double, starting from rank 0's, and rounded once.  No float
 *     atomics; every rank gets the same bits; with n = 1 the result is the tied trainer's bits.  The partials ride the backward gathers the
 *     sharded step already issues (one per tower layer, one for the heads): no collective is added.
 *   The solver step of the configured kind (vanilla, L2 / clip, momentum, Adam) is taken once per element with that sum, by the same code on
 *     every rank: parameters, velocity, moments and t stay replicated, nothing is broadcast.
 * agz_trainer_is_tied reports 1, agz_trainer_shard this rank's rows.  On such a handle:
 *   forward_backward(_dev), batch, train, train_dev, eval(_dev), export, save are COLLECTIVE as on an agz_trainer_create_sharded handle
 *     (planes / pi / v: this rank's B rows; train / train_dev: the global tensors).  save: rank 0 writes, byte for byte, the "AGZTRN05" file a
 *     single-process tied trainer with the global conf writes in the same state.
 *   init_random, set / get_param, get_grad, set / get_velocity, set / get_moments, apply, set_solver, set_adam, set_bn_tracking, load are
 *     local and take or give whole tied tensors, identical on every rank (every rank makes the same calls).  init_random(seed) draws what
 *     agz_trainer_create_tied with the global conf draws (the Glorot fans use the global BatchSize); load reads a tied file whose conf carries
 *     the global BatchSize (a plain trainer's file is AGZ_E_INVALID and leaves the handle untouched, as a tied file does on a plain sharded
 *     handle).
 *   agz_trainer_allreduce and agz_trainer_forward_backward_allreduce(_dev) return AGZ_E_STATE.
 * Errors of a collective call: as agz_trainer_create_sharded.  After a FUSED step (batch, train, train_dev) that fails part-way the ranks may
 * have stepped different layers: the replicated state may then differ between the ranks, and EVERY rank must reload a checkpoint before it
 * trains on.  Tests: tests/test_tied_sharded_cpu.py, tests/test_tied_sharded_gpu.py. */
int agz_trainer_create_sharded_tied(agz_comm* comm, const agz_net_conf* conf, agz_trainer** out);
/* this rank's rows of the global batch: [*row0, *row0 + *rows) of *n_ranks * *rows; a plain trainer reports 0, BatchSize, 1 */
int agz_trainer_shard(const agz_trainer* t, int* row0, int* rows, int* n_ranks);

#ifdef __cplusplus
}
#endif
#endif /* AGZ_H */
