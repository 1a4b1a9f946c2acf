/*
 * agz_debug.h — measurement and test hooks of libagz.so.  NOT part of the drop-in surface (include/agz.h): nothing on the
 * reference side binds these; bench.py reads the kernel-class timers, the parity tests read single Winograd stages.
 */
#ifndef AGZ_DEBUG_H
#define AGZ_DEBUG_H

#include "agz.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kernel-class timers: HIP events recorded on the ctx stream around every launch of a class.
 * enable=1 starts collecting (and clears), enable=0 stops.  agz_ctx_prof_read syncs and returns
 * the launch count and summed milliseconds of one class. */
#define AGZ_PROF_CONV 0    /* fused dual-branch 3x3 conv block launches (the dominant kernel) */
#define AGZ_PROF_HEADS 1   /* policy/value head kernel */
#define AGZ_PROF_SELECT 2  /* MCTS select/apply/encode */
#define AGZ_PROF_EXPAND 3  /* MCTS expand/backup */
#define AGZ_PROF_MOVE 4    /* root update / best move / apply */
#define AGZ_PROF_CONV_INIT 5 /* the single F->K input conv */
#define AGZ_PROF_WINO_IN 6   /* AGZ_COMPUTE_WINO: input transform; these three nest inside AGZ_PROF_CONV (the whole block) */
#define AGZ_PROF_WINO_GEMM 7 /* the 36 transform-domain GEMMs (the dominant kernel of that mode) */
#define AGZ_PROF_WINO_OUT 8  /* output transform + block epilogue */
#define AGZ_PROF_NCLASS 9
/* enable: 0 stop, 1 all classes, otherwise a mask with bit (k + 1) selecting class k (fewer event records per step) */
int agz_ctx_prof_enable(agz_ctx* ctx, int enable);
int agz_ctx_prof_read(agz_ctx* ctx, int klass, int64_t* launches, double* total_ms);
/* bracket only every stride-th launch of class klass (default 1): two event records per bracketed launch cost GPU time, and a
 * timed region that wants a kernel's average duration does not need every launch */
int agz_ctx_prof_set_stride(agz_ctx* ctx, int klass, int stride);

/* Diagnostics (tests): the first two stages of the Winograd path on host data.  x [B][H][W][C] (NHWC, C % 16 == 0),
 * w [N][C][3][3]  ->  V [36][T][C] = Bt d B of every 6x6 input tile, M [36][T][N] = V[pos] * (G g Gt)[pos],
 * T = B * ceil(H/4) * ceil(W/4) tiles in (board, tile row, tile column) order, pos = 6 * xi + nu. */
int agz_wino_stages(agz_ctx* ctx, const float* x, const float* w, int B, int H, int W, int C, int N, float* V, float* M);

/* Measurement: the Winograd tile size m (F(m x m, 3x3), m = 4 or 5) AGZ_COMPUTE_WINO_H2 uses on an H x W board — the one with
 * the fewest transform-domain rows, (m + 2)^2 * ceil(H/m) * ceil(W/m); bench.py prices the kernels' algorithmic bytes with it. */
int agz_wino_h2_tile(int H, int W);

/* Measurement: 1 when AGZ_COMPUTE_WINO_H2 runs the chained block (GEMM + fused out->in kernel, conv_wino_h2c.hpp) on an H x W board with K
 * filters, 0 when it runs the three-kernel block — bench.py prices the kernels' algorithmic bytes accordingly. */
int agz_wino_h2_chained(int H, int W, int K);

/* A/B hook: which form of the AGZ_COMPUTE_WINO_H2 block a net runs.  -1 (default): the chained form (output transform of block l
 * and input transform of block l+1 in one kernel, conv_wino_h2c.hpp) wherever the shape allows, else the three-kernel block;
 * 0: the three-kernel block; 1: as -1.  The environment switch AGZ_WINO_H2_FORM=0 (agz.h) does the same for a whole process. */
int agz_net_set_wino_h2_form(agz_net* net, int form);

/* A/B hook: which GEMM kernel the chained AGZ_COMPUTE_WINO_H2 block runs.  0 (default): the build's default; 1: wino_gemm_h2g_kernel
 * (128 x 256 tile, both operands streamed, three workgroups per CU); 2: wino_gemm_h2p_kernel (persistent, the weight slab stationary in
 * registers, M stores under the next tile's arithmetic; K = 256 only, other shapes keep kernel 1).  Results are bit-identical.  The
 * environment switch AGZ_WINO_H2_GEMM=1|2 (agz.h) does the same for a whole process.  Decomposition runs (timing only, the results are
 * NOT valid): 2 + 16 * mode with mode bit 0 = kernel 2 without its M stores, bit 1 = without its operand DMA (profiles/r05).
 * + 64 (with 0, 1 or 2): M and V2c stored with the default cache policy, as in round 4, instead of non-temporally (bit-identical; A/B).
 * + 128 (with 0, 1 or 2, and with + 64): every transform-domain row is kept — by default the tower's default kernels neither store,
 * multiply nor read the rows that only feed off-board outputs (the last transform point of the tiles that hang over the board's
 * edge: DESIGN 4a, gemm_maps.hpp); kernel 2 and the other forms always keep every row (bit-identical; A/B). */
int agz_net_set_wino_h2_gemm(agz_net* net, int variant);

/* What the last chained AGZ_COMPUTE_WINO_H2 block this net launched ran with: the live rows per 128-row slot at the class R (xi == AL-1)
 * and class C (nu == AL-1) positions, 0 = no such class / every row kept (19x19: 96, 96; with + 128 above, the persistent GEMM or the
 * other forms: 0, 0).  Lets a test see that the short positions are on, which identical results alone cannot show. */
int agz_net_wino_h2_last_rows(agz_net* net, int* live_r, int* live_c);

/* prepareRoot (mcts/search.go:392-408) evaluates the network only for roots without children.  agz_arena_begin_move packs those roots to
 * the front of the batch and runs the forward on the smallest batch that takes the same kernels as the arena's whole batch (per board the
 * results are bit-identical); on = 0 restores the whole-batch forward (A/B and parity hook).  agz_arena_last_prep_batch: boards the last
 * begin_move's forward ran on (0: skipped, no root needed it) and roots it had to evaluate. */
int agz_arena_set_prep_compact(agz_arena* arena, int on);
int agz_arena_last_prep_batch(agz_arena* arena, int* boards, int* roots);

/* Playout cap (agz_arena_set_playout_cap): past fast_budget only the FULL games of a move still search.  With one lane, one shared net and a
 * smaller batch that takes the whole batch's kernels, such a tail step packs them to the front of the network batch (per board the results
 * are bit-identical); on = 0 keeps the whole-arena batch (A/B and parity hook), default on.  agz_arena_last_cap_batch: the network batch
 * (boards) and the number of still-searching games of the last simulation step if it was a tail step; both 0 when it was not (a step within
 * fast_budget, prepareRoot, or a move without FULL games, whose tail is not enqueued). */
int agz_arena_set_cap_compact(agz_arena* arena, int on);
int agz_arena_last_cap_batch(agz_arena* arena, int* boards, int* games);

/* The split step.  Where one shared AGZ_INF_NET net runs the chained AGZ_COMPUTE_WINO_H2 tower of the arena's batch as two half-batch chains
 * on two queues (agz_net_set_tower_queues != 1, from 256 games by default), no lane rounds, no callback inferencer and no kernel-class
 * timer other than AGZ_PROF_MOVE running, agz_arena_simulate enqueues games [0, G/2) and [G/2, G) as two pipelines — select, network half,
 * expand — on the context's two queues with no event between them, the second half a tower behind the first; the queues are joined
 * lazily, by whatever next uses the context's stream (agz_ctx_sync included).  Results are bit-identical to the joined step.
 * mode 0: the joined step everywhere (A/B and parity hook); 1 (default): split, free-running after the first step's skew; 2: split with
 * the skew held by two events per step.  agz_arena_split_steps: simulation steps that took the split / the joined path since the arena
 * was created, and whether the last one was split (any pointer may be NULL). */
int agz_arena_set_split(agz_arena* arena, int mode);
int agz_arena_split_steps(agz_arena* arena, int64_t* split, int64_t* joined, int* last_split);

/* A/B hook: the trainer's AGZ_COMPUTE_WINO_H2 forward convolutions through the DMA GEMM on pre-split fp16 planes (k_conv_h2dma, train.hip;
 * default on) or through conv3x3_h2w_kernel, which splits the fp32 activations while staging them (bit 0 of `on` clear).  Bit 2 of `on` set:
 * the first form of the head kernels (one thread per output, three-block BatchNorm passes) instead of the second (default).  Bit 3 set: every
 * layer's weight images (fp16 hi / lo filter image of the forward convolution, Winograd image of the data gradient) built per layer in line
 * instead of at the start of the step on the trainer's side stream (default).  Bit 4 set: no side stream at all
 * (diagnostic: per-kernel durations without overlap).  Bit 5 set: the DMA forward convolution with one tap per K step (k_conv_h2dma, 128 x 256
 * tile) instead of nine taps from one x image (k_conv_h2dma3, 256 x 128 tile; default where the image fits its 372 rows).  Same tolerance;
 * bits 3, 4 and 5 do not change a single product.  Bits 6, 7: decomposition runs of k_conv_h2dma3 (no x image after chunk 0 / no weight DMA):
 * WRONG results, timing only.  Bit 8 (round 6): the weight gradient k_wgrad_h2t3 at two workgroups per CU as in round 5 (default: ONE — it then leaves
 * half of every SIMD's registers to the main stream's chain, which runs beside it).  Bit 9: the side stream at the lowest priority (set before
 * the first step; measured no different).  Bits 8 and 9 do not change a single product. */
int agz_trainer_set_dma_forward(agz_trainer* t, int on);

/* Tests: which kernels the trainer's last step (agz_trainer_forward_backward / _batch / _eval) launched for tower layer `layer`
 * (0 = the input convolution, 1 .. SharedLayers = the dual blocks).  Every value is written by the launcher at the very branch that
 * launches the kernel, so a test can see which of the shape-dependent paths a geometry took — identical results cannot show that.
 * Read-only: it has no effect on any launch.  0 = nothing launched (a layer before its first step; the data gradient of layer 0,
 * which has none; everything but the forward value after an eval). */
#define AGZ_PATH_FWD_F32 1      /* conv3x3_raw: the fp32-MFMA convolution */
#define AGZ_PATH_FWD_BF16X3 2   /* conv3x3_raw_x3 */
#define AGZ_PATH_FWD_H2W 3      /* conv3x3_raw_h2: conv3x3_h2w_kernel, activations split while staged */
#define AGZ_PATH_FWD_H2DMA 4    /* k_conv_h2dma: DMA GEMM on pre-split planes, one tap per K step, 128 x 256 tile */
#define AGZ_PATH_FWD_H2DMA3 5   /* k_conv_h2dma3: nine taps from one x image, 256 x 128 tile */
#define AGZ_PATH_WGRAD_F32 1    /* k_wgrad */
#define AGZ_PATH_WGRAD_X3 2     /* k_wgrad_x3 */
#define AGZ_PATH_WGRAD_H2 3     /* k_wgrad_h2 */
#define AGZ_PATH_WGRAD_H2T3 4   /* k_wgrad_h2t3: three taps per workgroup from hi / lo planes (boards >= 16 wide) */
#define AGZ_PATH_DGRAD_RAW 1    /* conv3x3_raw on the transposed filter */
#define AGZ_PATH_DGRAD_X3 2     /* conv3x3_raw_x3 */
#define AGZ_PATH_DGRAD_WINO_H2 3 /* conv3x3_raw_wino_h2 */
#define AGZ_PATH_BN2_SCALAR 1   /* k_bn_bwd2 (the weight gradient then takes dz's range with k_absmax) */
#define AGZ_PATH_BN2_V 2        /* k_bn_bwd2_v: vector form, writes dz's range itself */
int agz_trainer_last_paths(agz_trainer* t, int layer, int* fwd, int* wgrad, int* dgrad, int* bn_bwd2);

/* Tests: the row plan of the trainer's last step (agz_trainer_forward_backward / _batch) — how the kernels whose loops are sized by the
 * batch (M = B * H * W rows, B boards) were dealt their rows.  Every value is a copy of the very number the launcher passed to the kernel or
 * used as its grid; nothing is computed for the report and it has no effect on any launch.  A test restates the rules and compares, so that
 * a changed constant (rows per workgroup, a grid cap, the single-pass threshold) cannot silently move a shape back to a loop of one round.
 * layer 0 .. SharedLayers, out[AGZ_ROWS_*]:
 *   WGRAD_CHUNKS       chunks of the weight gradient's reduction: row chunks of 2048 rows for k_wgrad / k_wgrad_x3 / k_wgrad_h2
 *                      (ceil(M / 2048)), chunks of whole boards for k_wgrad_h2t3
 *   SINGLE_PASS        1: the BatchNorm statistics came from k_bn_stats + k_bn_fin2 (M >= 4096), 0: from the two k_bn_sum passes
 *   APPLY_RPB          rows per workgroup of k_bn_apply_v; 0 when the scalar k_bn_apply ran
 *   BWD2_RPB           rows per workgroup of k_bn_bwd2_v; 0 when the scalar k_bn_bwd2 ran
 *   APPLY_BOARD_WORDS  1: k_bn_apply_v also wrote per-board range words (its rows per workgroup <= H * W)
 *   BWD2_BOARD_WORDS   the same for k_bn_bwd2_v
 *   SPLIT_BLOCKS       workgroups the fp16x2 weight gradient's range / split passes over dz were launched with (k_absmax, k_split_h2,
 *                      k_split_h2p); 0 when the layer's weight gradient took no split pass
 *   SPLIT_NEED         workgroups those passes would take at one vector of four per thread: SPLIT_BLOCKS < SPLIT_NEED means they strided
 * layer SharedLayers + 1 reports the heads, out[AGZ_ROWS_HEAD_*]: SECOND_FORM 1 when the second form of the head kernels ran, then the grids
 * of k_head_conv2, k_head_stats_part (k_head_bn_bwd_a runs on the same grid) and k_cost_part (0 under AGZ_LOSS_ALPHAZERO); all 0 after a
 * step in the first form.  Unused words are 0.  After an eval the backward fields still hold the last training step's. */
#define AGZ_ROWS_WGRAD_CHUNKS 0
#define AGZ_ROWS_SINGLE_PASS 1
#define AGZ_ROWS_APPLY_RPB 2
#define AGZ_ROWS_BWD2_RPB 3
#define AGZ_ROWS_APPLY_BOARD_WORDS 4
#define AGZ_ROWS_BWD2_BOARD_WORDS 5
#define AGZ_ROWS_SPLIT_BLOCKS 6
#define AGZ_ROWS_SPLIT_NEED 7
#define AGZ_ROWS_HEAD_SECOND_FORM 0
#define AGZ_ROWS_HEAD_CONV2_GRID 1
#define AGZ_ROWS_HEAD_STATS_GRID 2
#define AGZ_ROWS_HEAD_COST_GRID 3
int agz_trainer_last_rows(agz_trainer* t, int layer, int32_t out[8]);

/* Tests: how tower layer `layer` (0 .. SharedLayers) came by the fp16 hi / lo planes of its input in the trainer's last step
 * (agz_trainer_forward_backward / _batch / _eval).  In AGZ_COMPUTE_WINO_H2 mode the vector BatchNorm pass of layer l - 1 writes them under
 * LAST step's range word of the tensor, and k_split_h2p_cond keeps them when that word and this step's exact one prescribe the same power
 * of two, else splits the tensor again (train.hip).  fused: 1 when the planes were written by the previous layer's BatchNorm pass and the
 * layer's forward convolution read planes (the host's planes_fused[layer] && x_planes as they stood after the step), else 0.  est_bits:
 * the estimate, amax_prev[2 layer + 1] — the bits of last step's max|x|.  range_bits: amax_words[2 layer + 1], this step's.  The planes
 * were kept iff fused && est_bits != 0 && both words give the same scale exponent (tests/test_train_history_gpu.py restates the rule).
 * Both words are zero for layers that never had them.  Synchronises and copies two words; launches nothing and has no effect on any
 * launch.  Lets a test see whether a layer kept or re-split its planes, which identical results cannot show. */
int agz_trainer_last_planes(agz_trainer* t, int layer, int* fused, uint32_t* est_bits, uint32_t* range_bits);

/* Tests: which kernels the last whole-batch forward of a net (agz_net_infer / agz_net_infer_dev, the arena's joined step) launched for the
 * input convolution, the dual blocks and the heads.  Every value is written on the host at the very branch of agz_net::forward_packed that
 * launches the kernel; read-only, no effect on any launch.  0 = nothing launched yet (block: also a net without blocks). */
#define AGZ_NPATH_IN_LAT 1                /* lat_input_kernel: latency regime, one launch with the first block's range words */
#define AGZ_NPATH_IN_X3 2                 /* conv3x3_x3_kernel<false>: bf16x3 products (the split modes, K % 128 == 0) */
#define AGZ_NPATH_IN_F32_411 3            /* launch_conv<4,1,1>: K % 64 != 0 (split-K inside it in the latency regime, as for the two below) */
#define AGZ_NPATH_IN_F32_221 4            /* launch_conv<2,2,1>: 64-row half tiles */
#define AGZ_NPATH_IN_F32_222 5            /* launch_conv<2,2,2> */
#define AGZ_NPATH_BLK_F32_411 1           /* launch_conv<4,1,1,true> */
#define AGZ_NPATH_BLK_F32_221 2           /* launch_conv<2,2,1,true> */
#define AGZ_NPATH_BLK_F32_222 3           /* launch_conv<2,2,2,true> */
#define AGZ_NPATH_BLK_F32_411_SPLITK 4    /* the same three with split-K and splitk_epilogue_kernel (latency regime, fp32) */
#define AGZ_NPATH_BLK_F32_221_SPLITK 5
#define AGZ_NPATH_BLK_F32_222_SPLITK 6
#define AGZ_NPATH_BLK_X3 7                /* conv3x3_x3_kernel<true> */
#define AGZ_NPATH_BLK_H2W 8               /* conv3x3_h2w_kernel (128 x 256 tile) */
#define AGZ_NPATH_BLK_H2 9                /* conv3x3_h2_kernel */
#define AGZ_NPATH_BLK_WINO 10             /* wino_launch: F(4x4,3x3), bf16x3 */
#define AGZ_NPATH_BLK_WINO_H2_3K 11       /* three-kernel Winograd fp16x2 block, 128 x 128 GEMM tile */
#define AGZ_NPATH_BLK_WINO_H2_3K_WIDE 12  /* ... 128 x 256 GEMM tile */
#define AGZ_NPATH_BLK_WINO_H2_CHAINED 13  /* chained Winograd fp16x2 block (conv_wino_h2c.hpp) */
#define AGZ_NPATH_BLK_LAT_H2 14           /* conv_lat_h2_launch: latency regime, one launch per block */
#define AGZ_NPATH_HEADS_ONE 1             /* heads_kernel: one workgroup per board */
#define AGZ_NPATH_HEADS_SPREAD 2          /* heads_feat / heads_fc / heads_out */
#define AGZ_NPATH_HEADS_SPREAD_NB4 3      /* ... with heads_fc_nb_kernel<4> (from 32 boards) */
int agz_net_last_paths(agz_net* net, int* input_conv, int* block, int* heads);

/* Tests: the tensor the heads of the last agz_net_infer / agz_net_infer_dev of B boards read — the tower's output — unpacked on the host
 * from the padded NHWC device layout [B][Hp][Wp][Kp] to host[B][K][H][W].  Synchronises and copies; launches nothing.  AGZ_E_STATE before
 * the first forward and after a split step (forward_half), which clears the record. */
int agz_net_tower_out(agz_net* net, int B, float* host);

/* The smallest batch >= n that runs the kernels of a batch of G boards on this net in its current compute mode (agz_net::min_same_batch, what
 * prepareRoot's packed forward uses): per board the outputs of such a batch are those of the G-board batch bit for bit.  The parity tests
 * evaluate single leaves for the oracle with it instead of G copies of the board. */
int agz_net_min_same_batch(agz_net* net, int n, int G, int* batch);

/* Measurement: raw device counter `which` of an arena.  AGZ_CNT_PATHMAX: nodes on the LONGEST descent since the last reset (all games run
 * one simulation per step in lock step: a step's k_select lasts as long as its longest path, so the maximum — not the mean that
 * agz_arena_stats reports — is what prices the kernel on narrow, deep trees). */
#define AGZ_CNT_PATHMAX 15
int agz_arena_debug_counter(agz_arena* arena, int which, int64_t* value);

/* Measurement: the node-pool capacity of an arena's trees and how often AGZ_POOL_GROW has re-allocated them */
int agz_arena_pool_capacity(agz_arena* arena, int* nodes_per_pool, int* grows);

/* Tests: the size of the device staging buffer and of each of the two page-locked host buffers agz_arena_save / agz_arena_load stream the
 * nodes and example rows through (default 256 MB; 64 bytes .. 4 GiB).  A few hundred bytes force many chunks, and trees cut across chunks,
 * at tiny shapes.  The file does not depend on it. */
int agz_arena_set_ckpt_staging(agz_arena* arena, size_t bytes);

/* Tests: the same for agz_replay_save / agz_replay_load (default 256 MB; 4 bytes .. 4 GiB).  A chunk holds as many whole rows of the array
 * being moved as fit, at least one: the bytes of three rows of planes cut chunks inside every array and across the ring's wrap at toy
 * sizes.  The file does not depend on it. */
int agz_replay_set_ckpt_staging(agz_replay* rp, size_t bytes);

/* Failure injection (tests): the data-parallel step of this communicator fails on THIS rank right before it would enter the collective of
 * slice k (0 = the heads, 1 .. = layer L .. 0; k < 0: off).  One shot: cleared by the step it hits.  What the test checks is the rule of
 * agz_trainer_forward_backward_allreduce: the failing rank still enters every collective, every rank's call fails (AGZ_E_PEER on the
 * healthy ones), nobody hangs, and the next step is a normal one. */
int agz_comm_debug_fail_slice(agz_comm* comm, int k);

/* Failure injection (tests): the next collective step of a sharded trainer on this communicator (agz_trainer_create_sharded) returns an
 * error on THIS rank right before the first exchange of tower layer `layer` (0 .. SharedLayers; SharedLayers + 1 = the heads; < 0: off) —
 * an error return, nothing on the device.  One shot.  What the test checks: the failing rank still enters every remaining collective of
 * the step, every rank's call fails (AGZ_E_PEER on the healthy ones), nobody hangs, and the next step is a normal one. */
int agz_comm_debug_fail_layer(agz_comm* comm, int layer);

#ifdef __cplusplus
}
#endif
#endif /* AGZ_DEBUG_H */
