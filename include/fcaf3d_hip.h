/* libfcaf3d_hip.so — C ABI of the MI355X-native FCAF3D sparse-voxel hot path.
 *
 * Every entry point takes raw DEVICE pointers, explicit sizes and a hipStream_t, enqueues its
 * kernels on that stream and returns immediately:
 *     0  = ok,  <0 = invalid argument (-1) / workspace too small (-2),  >0 = hipError_t.
 * The library never allocates device memory: data-dependent output sizes come back through a
 * device counter (`*_dev`), and scratch space is passed in (`ws`, size from the matching
 * `*_ws_bytes`).  (It owns a handful of hipEvents: fc_exec, fc_plan_*.)  It never calls exit() (contrast mmdet3d/ops/pcdet_nms/src/iou3d_nms.cpp:14-38).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference
 * repository; "ME" = MinkowskiEngine v0.5.4, the un-vendored dependency pinned at
 * docker/Dockerfile:27-32, named by its Python call site).
 *
 * Layouts: coords int32 (N,4) = [batch, x, y, z] in voxel units (multiples of the tensor stride);
 * features fp32 (N,C) row-major; conv kernels fp32 (K,Cin,Cout) with offsets x-fastest;
 * neighbour tables int32 (K,N_out), -1 = absent; voxel hash = open addressing over 64-bit packed
 * keys (`cap` a power of two >= 2N) with int32 values = row index.
 */
#ifndef FCAF3D_HIP_H
#define FCAF3D_HIP_H
#include <stdint.h>

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this ABI (No reference counterpart): bumped whenever a prototype or the meaning of a flag bit changes — r5 -> 5
 * (flags bit27 went from "input is pre-split planes" to "flat addressing", fc_x6_planes / fc_conv_x6d removed: ADVICE r5),
 * r6 -> 6 (fc_compact_rows takes the output capacity; fc_plan_*, fc_argsort27 added), r6 -> 7 (fc_set_split_mode / fc_get_split_mode / fc_amax /
 * fc_conv_amax_hint / fc_amax_out_hint added; weight images are mode-dependent and fc_x6_weight_images writes their amax word), -> 8
 * (fc_merge_sorted_segments / fc_merge_sorted_segments_ws_bytes added: test-time augmentation), -> 9 (fc_norm_act_maxpool8_fwd / fc_maxpool8_norm_act_bwd / fc_inverse_rows / fc_norm_act_add_fwd /
 * fc_bn_train_add_fwd added: the stem's tail and the neck's sparse sums without their intermediates), -> 10 (fc_conv_fwd_route /
 * fc_conv_wgrad_route added: the launch a convolution call becomes, as data), -> 11 (fc_bn_train_fwd_route / fc_bn_train_bwd_route
 * added: the launches a normalisation call becomes, as data), -> 12 (fc_eval_match / fc_eval_match_ws_bytes added: the matching
 * of indoor_eval on the device), -> 13 (fc_eiou3d_fwd_bwd added: the enclosing-box losses GIoU3DLoss / DIoU3DLoss), -> 14
 * (fc_batch_augment_voxelize added: the input pipeline of a whole batch from a resident arena in one launch), -> 15
 * (fc_norm_act_maxpool8_mask_fwd / fc_maxpool8_mask_norm_act_bwd added: the stem's tail with a per-child arg-max mask), -> 16 (fc_adamw_groups_table_bytes /
 * fc_adamw_groups_pack / fc_adamw_step_groups added: AdamW with per-parameter rate and decay multipliers), -> 17 (fc_bn_eval_bwd / fc_bn_eval_bwd_ws_bytes /
 * fc_bn_eval_bwd_route added: the backward through a BatchNorm that reads its running statistics), -> 18 (fc_x6_weight_images takes the
 * grid of its amax pass, amax_chunks / amax_blocks; fc_x6_amax_units / fc_x6_weight_images_passes added), -> 19 (fc_vote_boxes added: box
 * voting between the merge NMS and the per-scene merge of test-time augmentation).  fc_adamw_ema_step / fc_swap_f32
 * (AdamW with the weight average of mmcv's EMAHook in the same launch, the exchange of two flat buffers) were added at 19 WITHOUT a
 * bump: nothing existing changed, tests/test_vote_cpu.py pins 19, and a library that lacks a declared symbol is refused by
 * _lib.lib() whatever its version.  fc_grad_accum / fc_grad_accum_norm / fc_grad_accum_norm_ws_bytes (gradient accumulation over
 * the flat buffers) were added the same way, for the same reason.  A caller built against
 * another version must not go on: tests/test_cabi.py pins the number the Python host was written for. */
#define FC_ABI_VERSION 19
#ifndef FC_AMAX_SLOT_BYTES
#define FC_AMAX_SLOT_BYTES 2048
#endif
int fc_abi_version(void);

/* ---- coordinates -------------------------------------------------------------------------- */

/* ME.utils.batch_sparse_collate quantisation of one scene — single_stage_sparse.py:34-36.
 * coords[i] = [batch_idx, floor(xyz/voxel_size)], feats[i] = points[i,3:3+nfeat] / feat_div. */
int fc_voxelize(const float* points, int64_t n, int pt_stride, int batch_idx, float voxel_size, float feat_div,
                int nfeat, int* coords, float* feats, hipStream_t stream);

/* The reference's indoor TRAIN pipeline fused with the collate above, one pass over the raw points of a scene:
 * GlobalAlignment (mmdet3d/datasets/pipelines/transforms_3d.py:409-490), IndoorPointSample (:821-895, sample_idx: n_out
 * row indices, nullable = every row), RandomFlip3D (:59-170), GlobalRotScaleTrans (:493-645), then
 * ME.utils.batch_sparse_collate's floor(xyz / voxel_size) and features / feat_div (single_stage_sparse.py:34-36).
 * xform_host: 24 floats on the HOST — [0..8] alignment R row-major, [9..11] t, [12] has_align, [13] flip x, [14] flip y,
 * [15] cos(angle), [16] sin(angle), [17] scale, [18..20] translation, [21..23] unused.  points_out (nullable):
 * the augmented cloud (n_out, 3 + nfeat), for inspection — the detector itself needs coords / feats only. */
int fc_augment_voxelize(const float* points, int64_t n_src, int pt_stride, const int* sample_idx, int64_t n_out,
                        const float* xform_host, int batch_idx, float voxel_size, float feat_div, int nfeat, int* coords,
                        float* feats, float* points_out, hipStream_t stream);

/* The same train pipeline for ALL B scenes of a batch in one launch, with the sampling drawn in the kernel: IndoorPointSample
 * (mmdet3d/datasets/pipelines/transforms_3d.py:821-895), GlobalAlignment (:409-490), RandomFlip3D (:59-170), GlobalRotScaleTrans
 * (:493-645) and the collate of extract_feat (mmdet3d/models/detectors/single_stage_sparse.py:34-36), from a resident arena of raw points
 * (arena_rows, pt_stride) fp32 that holds many scenes back to back.  desc: DEVICE table of B <= 256 scenes, FC_BATCH_DESC_WORDS
 * int64 words each: [0] first arena row, [1] n_src, [2] n_out, [3] first output row, [4] 64-bit sample seed, [5] first entry in
 * sample_idx, [6..17] the 24 floats of fc_augment_voxelize's xform_host.  Scene s writes rows [out_off, out_off + n_out) of
 * coords (batch index s) / feats / sample_out / points_out (each out_rows rows; rows outside every scene's range are not
 * touched).  Row j of a scene reads source row perm_seed(j), a keyed bijection of [0, n_src) (four-round Feistel network with
 * cycle walking: n_out distinct rows), or with n_src < n_out a keyed hash of j reduced to [0, n_src) (with replacement), or —
 * sample_idx != NULL (n_idx ints) — sample_idx[idx_off + j]; csrc_post/batch.hip states the integer arithmetic.  The arithmetic
 * behind the gather is fc_augment_voxelize's: coords / feats are bit-equal to B calls of it with the same rows.  total_out =
 * the sum of n_out as the HOST knows it (sizes the grid; 0, or B == 0: nothing is launched).  sample_out (nullable): the rows
 * chosen; points_out (nullable): the augmented cloud.  A descriptor whose ranges leave the arrays writes nothing. */
#define FC_BATCH_DESC_WORDS 18
int fc_batch_augment_voxelize(const float* arena, int64_t arena_rows, int pt_stride, const int64_t* desc, int B, int64_t total_out,
                              int64_t out_rows, const int* sample_idx, int64_t n_idx, float voxel_size, float feat_div, int nfeat,
                              int* coords, float* feats, int* sample_out, float* points_out, hipStream_t stream);

/* Z-order key per voxel coordinate [b | x,y,z bit-interleaved]; sorting the collated points by it before
 * fc_hash_unique turns "order of first occurrence" into a space-filling-curve order on every pyramid level.
 * No reference counterpart (optional locality aid of this implementation, off by default). */
int fc_morton_keys(const int* coords, int64_t n, long long* keys, hipStream_t stream);

/* Order-preserving compaction primitive (wave ballot + prefix sum): pos[i] = #set flags before i — the row selection
 * of ME.MinkowskiPruning (fcaf3d_neck_with_head.py:76, called at :124-125) and of the per-scene decomposition.
 * fc_compact_rows: kept has room for m entries (r6: set flags past that capacity are dropped, missing ones read 0). */
int fc_scan_flags(const unsigned char* flags, int64_t n, int* pos, int* total_dev, void* ws, int64_t ws_bytes,
                  hipStream_t stream);
int fc_compact_rows(const unsigned char* flags, const int* pos, int64_t n, int* kept, int64_t m, hipStream_t stream);

/* ME.SparseTensor(coordinates, features) de-duplication (single_stage_sparse.py:37) and the strided
 * output coordinate set of MinkowskiConvolution/MaxPooling(stride=2) (me_resnet.py:19-24,56-62):
 * unique rows of floor(coords/q)*q in order of first occurrence; builds the voxel hash of the
 * result (key -> row).  first_idx / inverse may be NULL.  Coordinates must lie in [-32639, 32639] per axis and the
 * batch index in [0, 32767] (64-bit packed hash keys, 16 bits per field): if any row does not — a stray outlier, an
 * inf coordinate — *n_out_dev is set to -1 and the set must not be used.  With q > 1 the rows are voxels of an accepted
 * set and the limit holds for the rounded voxel, whose lowest value is -32640 (what -32639 rounds down to). */
int64_t fc_hash_unique_ws_bytes(int64_t n);
int fc_hash_unique(const int* coords, int64_t n, int q, unsigned long long* table_keys, int* table_vals, int64_t cap,
                   int* out_coords, int* first_idx, int* inverse, int* n_out_dev, void* ws, int64_t ws_bytes,
                   hipStream_t stream);

/* ME CoordinateManager kernel map for one (in set, out set, kernel) triple: nbr[k][o] = input row at
 * out_coords[o] + offsets[k] — built inside every ME.MinkowskiConvolution / MinkowskiMaxPooling call
 * (me_resnet.py:19-24, :56-62; fcaf3d_neck_with_head.py:52, :69). */
int fc_kernel_map(const int* out_coords, int64_t n_out, const unsigned long long* table_keys, const int* table_vals,
                  int64_t cap, const int* offsets, int K, int* nbr, hipStream_t stream);
/* per-row occupancy masks of a neighbour table, and the table permuted into a row order (mask-sorted rows).
 * No reference counterpart: scheduling aid of the output-stationary kernel. */
int fc_nbr_row_masks(const int* nbr, int64_t n_out, int K, int* masks, hipStream_t stream);
int fc_permute_nbr(const int* nbr, const int* order, int64_t n_out, int K, int* nbr_sorted, hipStream_t stream);
/* exact (input row, output row) pair lists per kernel offset, ascending in the output row — what ME's kernel map
 * (in_maps / out_maps per offset; consumed by the convolutions of me_resnet.py:56-62) holds; the weight-gradient pass reduces over them (fc_conv_wgrad_pairs).
 * pair_in / pair_out are (K, n_out) int32 with the first cnt[k] entries of row k valid; pair_pos (nullable,
 * (K, n_out)) is the inverse: pair_pos[k][o] = j with pair_out[k][j] == o, or -1. */
int64_t fc_kernel_map_pairs_ws_bytes(int64_t n_out, int K);
int fc_kernel_map_pairs(const int* nbr, int64_t n_out, int K, int* pair_in, int* pair_out, int* pair_pos, int* cnt,
                        void* ws, int64_t ws_bytes, hipStream_t stream);
/* nbr_t[k][i] = o  iff  nbr[k][o] == i  (the gather table of the backward-data pass: ME's convolution backward walks the
 * same in/out maps with the roles swapped, `gin[i] += gout[o] @ W[k]^T`; reached by autograd of me_resnet.py:56-62). */
int fc_kernel_map_transpose(const int* nbr, int64_t n_out, int64_t n_in, int K, int* nbr_t, hipStream_t stream);

/* ME.MinkowskiGenerativeConvolutionTranspose(k=2,s=2) output coordinates — fcaf3d_neck_with_head.py:60-66:
 * out[8i+k] = coords[i] + {0,half_stride}^3 (x fastest). */
int fc_gen_coords(const int* coords, int64_t n, int half_stride, int* out_coords, hipStream_t stream);

/* Kernel map and membership of a GENERATED children set (the output set of ME.MinkowskiGenerativeConvolutionTranspose,
 * fcaf3d_neck_with_head.py:60-66, on which the neck's k3 convolutions run, :52, :69) from the PARENT level by index
 * arithmetic instead of hash probes: child k of parent row i sits at row 8i + k.
 *   fc_kernel_map_children: nbr (27, 8 n_parent) of the children set onto itself (k3 s1) from the parent set's own
 *     k3 s1 table parent_nbr (27, n_parent) — identical to fc_kernel_map on the children's hash;
 *   fc_child_rows: row of each query voxel (stride T) in the children set of the set behind the parent table (stride 2T),
 *     -1 if its parent cell is absent; *n_found_dev = number of hits — what the sparse `a + b` union (:101) needs when
 *     the backbone level lies inside the generated set. */
int fc_kernel_map_children(const int* parent_nbr, int64_t n_parent, int* nbr, hipStream_t stream);
int fc_child_rows(const int* query_coords, int64_t n, const unsigned long long* parent_keys, const int* parent_vals,
                  int64_t cap, int child_stride, int* rows, int* n_found_dev, hipStream_t stream);

/* SparseTensor `a + b` on different coordinate maps — fcaf3d_neck_with_head.py:101: row of every b
 * voxel in the union (a's rows first, then b's new voxels in order); new_coords gets b's new rows. */
int64_t fc_union_map_ws_bytes(int64_t n_b);
int fc_union_map(const int* coords_b, int64_t n_b, const unsigned long long* table_keys_a, const int* table_vals_a,
                 int64_t cap_a, int64_t n_a, int* row_b, int* new_coords, int* n_new_dev, void* ws, int64_t ws_bytes,
                 hipStream_t stream);

/* SparseTensor.features_at_coordinates (MinkowskiInterpolation) — fcaf3d_neck_with_head.py:115-116. */
int fc_interp(const int* query_coords, int64_t n, const unsigned long long* table_keys, const int* table_vals, int64_t cap,
              const float* feats, int C, int tensor_stride, float* out, hipStream_t stream);

/* coordinate rows of a pruned set (MinkowskiPruning, fcaf3d_neck_with_head.py:125). */
int fc_gather_coords(const int* src, const int* idx, int64_t n, int* dst, hipStream_t stream);

/* ---- the coordinate phase of a step as two native calls (r6; csrc/plan.hip) ------------------------------------------------ */

/* SingleStageSparse3DDetector.extract_feat's collate + ME.SparseTensor (mmdet3d/models/detectors/single_stage_sparse.py:34-37) and
 * the coordinate sets behind every strided ME.MinkowskiConvolution / MinkowskiMaxPooling of the backbone (me_resnet.py:19-24,
 * :56-62) in ONE call: points of B scenes -> the sets [cm0, m1, m2, L1..Lnl] (strides 1, 2, 4, 8 ...), each with its voxel hash,
 * rows in order of first occurrence, level 0 with its feature rows.  The chain runs with device-resident row counts; the call
 * ends with its single host read-back (rows per set, rows per set and scene, range flags) and fills `out`.
 *   cfg (fc_plan_cfg_words() int64): the C_* words of fcaf3d_amd/csrc/plan_layout.h — sizes, voxel sizes (double bits), which tables
 *     are wanted, the row thresholds of the convolution routes, pts_threshold, optional pre-voxelised input (device pointers).
 *   scenes: B x {device pointer, points, floats per point} (int64).  arena1: fc_plan_stage1_bytes bytes of device memory.
 *   counts_host: PINNED host ints, METAW (3 + nl) + (3 + nl) B.  out: fc_plan_out_words int64.  Every word of cfg, out, the counts and
 * the counter block is declared in fcaf3d_amd/csrc/plan_layout.h (the text plan.hip compiles and fcaf3d_amd/plan.py reads).
 * fc_plan_maps, with those counts: every kernel map of the backbone and of the neck (fcaf3d_neck_with_head.py:52, :60-71, :101:
 * generated children sets and their maps by index arithmetic, union rows of the backbone levels), the derived tables of each
 * convolution route (mask-sorted tables, pair lists, transposed tables) and the head's location / scene / level arrays
 * (fcaf3d_neck_with_head.py:276-277) into arena2 (fc_plan_stage2_bytes), ending with ITS single read-back (pair-list counts, union
 * hits) into cnt_host (PINNED ints, CNT_MAP maps + CNT_TAIL + nl B + 1).  Same sets, tables and row orders as the per-operator entry points above.
 * fc_argsort27: the stable argsort of 27-bit occupancy masks used for the mask-sorted tables (No reference counterpart).
 * cfg[C_PROBE] != 0: every launch (group) of the two calls is bracketed with a HIP-event pair; fc_plan_probe_read(ms, bytes, kind, cap),
 * called after the device has drained, returns the brackets since the last read-out with their compulsory bytes and kind (PK_* of
 * plan_layout.h; fcaf3d_amd/plan.py PROBE_KINDS names them): bench.py's
 * `roofline.hbm_kernels` (the reference times whole iterations only: tools/analysis_tools/benchmark.py:64-91). */
int fc_plan_cfg_words(void);
int fc_plan_out_words(int B, int nl);
int64_t fc_plan_stage1_bytes(int64_t total_points, int B, int nl, int nfeat);
int fc_plan_levels(const int64_t* cfg, const int64_t* scenes, void* arena1, int64_t arena1_bytes, int64_t* out, int* counts_host,
                   hipStream_t stream);
int64_t fc_plan_stage2_bytes(const int64_t* cfg, int64_t* out, const int* counts_host);
int fc_plan_maps(const int64_t* cfg, int64_t* out, const int* counts_host, void* arena2, int64_t arena2_bytes, int* cnt_host,
                 hipStream_t stream);
int64_t fc_plan_probe_read(float* ms, double* bytes, int* kind, int64_t cap);
int64_t fc_argsort27_ws_bytes(int64_t n);
int fc_argsort27(const int* keys, int64_t n, int* order, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- sparse convolution ------------------------------------------------------------------- */

/* Bits of the `flags` word of the convolution entry points (fc_conv_fwd*, fc_conv_fwd_pairs*, fc_conv_wgrad*, the ws / stats size
 * queries) and of fc_exec_run's cfg[1].  0 is the default route; tools/nbench and tools/convbench.py sweep the variant bits. */
/* force the generic FMA kernels instead of the MFMA kernels (the parity cross-check) */
#define FC_CONV_FMA (1 << 0)
/* tuning fields, 0 = the plan's choice: bits 4-5 tile rows (1 = 64, 2 = 128, 3 = 256 x 64 tiles), bits 6-7 tile columns
 * (1 = 64, 2 = 128), bits 8-15 S, the number of partial sums (offsets per split for a convolution, row ranges for a weight gradient) */
#define FC_CONV_BM_SHIFT 4
#define FC_CONV_BN_SHIFT 6
#define FC_CONV_TILE_MASK 3
#define FC_CONV_S_SHIFT 8
#define FC_CONV_S_MASK 255
/* weight gradient: never the deeper-pipelined kernel k_wgrad_mfma_p (the r1 kernel) */
#define FC_CONV_WGRAD_PIPE_OFF (1 << 16)
/* convolution: the deeper-pipelined LDS kernel k_conv_mfma_p off / on (else chosen by the number of workgroups) */
#define FC_CONV_PIPE_OFF (1 << 17)
#define FC_CONV_PIPE_ON (1 << 18)
/* weight gradient over a table: 64-row chunks (ignored by fc_conv_wgrad_pairs) */
#define FC_CONV_WGRAD_DEEP (1 << 19)
/* weight gradient: k_wgrad_mfma_p wherever it applies */
#define FC_CONV_WGRAD_PIPE_ON (1 << 20)
/* convolution: the LDS-DMA kernel k_conv_glds (2 workgroups per CU) */
#define FC_CONV_GLDS (1 << 21)
/* convolution: offset-split launches of a dense table stay off the LDS-DMA kernel */
#define FC_CONV_GLDS_OFF (1 << 22)
/* fc_conv_fwd / fc_conv_fwd_pairs(_tiles), nbr != NULL: W[k] is stored TRANSPOSED, (Cout, Cin) row-major — the backward-data pass
 * run on the layer's own (K, Cin, Cout) kernel without a transposed copy */
#define FC_CONV_WT (1 << 23)
/* the same fp32 convolution (torch.float32 in and out, as ME.MinkowskiConvolution computes it, me_resnet.py:56-62) on the matrix
 * pipe by EXACT operand splitting — x = x1 + x2 + x3 with three 8-bit pieces, six bf16 x bf16 products (each exact in the fp32
 * accumulator) per fp32 product (the three dropped ones: <= 2^-24 of the product with the round-to-nearest split of r4), or in
 * split mode 2 two fp16 pieces and three products; results sit at fp32 rounding level against fp64, like the fp32 MFMA's
 * (csrc/conv_x6.h, tests/test_gpu_ops.py).  128- and 256-row tiles.  Weight gradients: the split kernels (csrc/wgrad_x6.h)
 * where one exists for the shape, the fp32 MFMA kernels otherwise. */
#define FC_CONV_SPLIT (1 << 24)
/* with FC_CONV_SPLIT: `W` is not the fp32 kernel but its pre-split image built by fc_x6_weight_image — for the backward-data pass
 * the image of the transposed operator (then FC_CONV_WT is not needed) */
#define FC_CONV_IMAGE (1 << 26)
/* with FC_CONV_SPLIT (r5): flat 64-bit addresses for the gathered rows and the image.  Without it a gathering launch whose `in`
 * ends below 2 GB (n_in Cin 4 bytes) reads both through buffer descriptors — a lane's row is a 32-bit byte offset computed once per
 * kernel offset, an absent neighbour an offset past the descriptor's end (the load returns zeros): the same loads, bit-identical
 * results, a third fewer address instructions per stage (csrc/conv_x6.h BUF).  Larger operands and table-free launches
 * (nbr == NULL) take the flat route by themselves.  The descriptor route addresses the weight image with 32-bit offsets: a caller
 * whose image reaches 4 GB (6 K Cin Cout bytes; 42 MB for the largest layer of the reference's networks) sets this bit. */
#define FC_CONV_FLAT (1 << 27)
/* weight gradient over a dense table: no multi-offset kernel k_wgrad_multi / restrict it to its first rule (Cin = 64, >= 32768 rows) */
#define FC_CONV_WGRAD_MULTI_OFF (1 << 29)
#define FC_CONV_WGRAD_MULTI_FIRST (1 << 30)

/* fc_x6_weight_image: image of W (K, R, C) — or, transposed != 0, of the operator W[k]^T where W[k] is stored (C, R) —
 * for a launch with Cin = R, Cout = C; R % 32 == 0, C % 64 == 0; fc_x6_weight_image_bytes(K, R, C) = 6 K R C bytes
 * (the operand of FC_CONV_IMAGE launches of ME.MinkowskiConvolution, me_resnet.py:56-62). */
int64_t fc_x6_weight_image_bytes(int K, int R, int C);
int fc_x6_weight_image(const float* W, void* img, int K, int R, int C, int transposed, hipStream_t stream);
/* The images of many kernels in ONE launch (all convolutions of a model — me_resnet.py:56-62, fcaf3d_neck_with_head.py:52,60-69 —
 * both directions, right after the optimizer step: the reference's optimizer hook, mmcv OptimizerHook.after_train_iter, is where
 * its weights change): `desc` is a DEVICE array
 * of n entries of 8 int64 {W pointer, image pointer, K, R, C, transposed, first block, sibling}; sibling (split mode 2): 0, or
 * the address of another image of the SAME weights listed earlier (the forward image of a backward-data entry) whose amax slot
 * this entry shares instead of making its own pass over W; entry e owns the blocks from its
 * first block up to the next entry's, K (R / 32) (C / 64) of them; total_blocks = the last entry's first block + its blocks.
 * amax_chunks (split mode 2; a DEVICE array of amax_blocks int64, built once by the caller): the grid of the amax pass, which runs
 * over the entries WITHOUT a sibling only — with U = fc_x6_amax_units(), an entry of u units (8 KB of weights each) lists its
 * ceil(u / U) chunks as  entry index << 32 | chunk,  one block of the pass each, in any order.  An entry with a sibling lists none. */
int64_t fc_x6_amax_units(void);
int fc_x6_weight_images(const int64_t* desc, int n, int64_t total_blocks, const int64_t* amax_chunks, int64_t amax_blocks,
                        hipStream_t stream);
/* the same with a choice of passes (No reference counterpart: measurement, tools/imgbench.py): bit 0 zero the amax slots, bit 1 the amax pass, bit 2 the image pass */
int fc_x6_weight_images_passes(const int64_t* desc, int n, int64_t total_blocks, const int64_t* amax_chunks, int64_t amax_blocks,
                               int passes, hipStream_t stream);

/* ME.MinkowskiConvolution forward (me_resnet.py:19-21,56-62; BasicBlock; fcaf3d_neck_with_head.py:52,69),
 * its backward-data pass (call with the transposed table and fc_transpose_weight'ed kernel), and with
 * nbr == NULL (K = 1, identity) the dense GEMMs of MinkowskiGenerativeConvolutionTranspose (:60-66)
 * and of the 1x1 head convolutions (:83-85, :257-263).  out[o] = sum_k in[nbr[k][o]] @ W[k].
 * `flags`: the FC_CONV_* bits above.  Layers with too few rows to fill
 * the chip are split over kernel offsets into `ws` and summed in a fixed order (deterministic).
 * out_index (nullable): `nbr` is a table permuted into occupancy-mask order (fc_permute_nbr) and tile row t
 * belongs to output row out_index[t] — tiles of similar rows skip the offsets none of them has. */
int64_t fc_conv_fwd_ws_bytes(int64_t n_out, int K, int Cin, int Cout, int flags);
int fc_conv_fwd(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ME.MinkowskiConvolution (me_resnet.py:56-62, BasicBlock convs; fcaf3d_neck_with_head.py:52) the way ME itself runs it
 * (per offset: gather -> GEMM -> scatter) over the exact pair lists:
 * T_k = in[pair_in[k][:cnt[k]]] @ W[k] into the workspace, then out[o] = sum_k T_k[pair_pos[k][o]] in fixed k order.
 * No MFMA work is issued for absent neighbours; pays off on the small, ~60 % occupied deep levels.  MFMA shapes only
 * (Cin % 32 == 0, Cout % 64 == 0).  For the backward-data pass pass the lists of the transposed table. */
int64_t fc_conv_fwd_pairs_ws_bytes(int64_t n_out, int K, int Cout);
int fc_conv_fwd_pairs(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                      float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, void* ws,
                      int64_t ws_bytes, hipStream_t stream);

/* The same (ME.MinkowskiConvolution per offset over its in/out maps, me_resnet.py:56-62) for a caller that has read the pair
 * counts back: live_tiles = sum_k ceil(pair_cnt[k] / 128) launches exactly the non-empty (offset, 128-row tile) workgroups
 * as one linear list (no workgroup exits on arrival; evenly filled shader engines).  live_tiles <= 0: as fc_conv_fwd_pairs. */
int fc_conv_fwd_pairs_tiles(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                            float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                            void* ws, int64_t ws_bytes, hipStream_t stream);

/* r5 — the convolution -> BatchNorm pairs of the network (BasicBlock conv1 / norm1, conv2 / norm2, me_resnet.py:3, :56-63; the
 * neck's blocks, fcaf3d_neck_with_head.py:52-53, :60-62, :66-68): fc_conv_fwd / fc_conv_fwd_pairs_tiles that ALSO leave, per row
 * block of their result, the column sums of the result and of its square — stats[fc_conv_stats_blocks(...)][2][Cout] — written
 * by whichever kernel produces the final rows (the MFMA tile epilogue, or the fixed-order sum of an offset-split / pair-list
 * launch).  fc_bn_train_fwd(part = stats) turns them into the batch statistics without reading the matrix again.  Split-bf16
 * route only (FC_CONV_SPLIT | FC_CONV_IMAGE); fc_conv_stats_blocks returns 0 where a launch has no statistics epilogue.  stats == NULL:
 * exactly the plain entry points. */
int64_t fc_conv_stats_blocks(int64_t n_out, int K, int Cin, int Cout, int flags, int pairs);
int fc_conv_fwd_stats(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                      int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, float* stats,
                      hipStream_t stream);
int fc_conv_fwd_pairs_tiles_stats(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                                  float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                                  void* ws, int64_t ws_bytes, float* stats, hipStream_t stream);
/* ... and the backward half of the same pairing (r5): the backward-data pass of a convolution whose INPUT came out of a BatchNorm
 * (+ ReLU / ELU, no residual: BasicBlock norm1 -> conv2, me_resnet.py:3; the neck's norm -> conv chains and out_block -> head,
 * fcaf3d_neck_with_head.py:52-71, :257-263) also leaves that layer's two backward reductions per row block —
 * stats[blocks][2][Cout] = column sums of g' = g act'(pre) and of g' xhat (pre, xhat from the layer's input bn_x (n_out, Cout) and
 * its batch mean / var / gamma / beta / eps; act 0 none, 1 ReLU, 2 ELU) — which fc_bn_train_bwd(part = stats) consumes instead of
 * reading bn_x and g once more.  add (nullable): a second contribution to that gradient, g = result + add (the layer's output had
 * two consumers: BasicBlock's `out += residual`); bn_y (nullable): the layer's output, from which act'(.) is taken when a residual
 * was added before the activation (norm2 of a BasicBlock; NULL: act' is recomputed from bn_x). */
int fc_conv_fwd_bn_bwd_stats(const float* in, const float* W, const int* nbr, const int* out_index, float* out, int64_t n_in,
                             int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, float* stats,
                             const float* bn_x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                             int act, const float* add, const float* bn_y, hipStream_t stream);
int fc_conv_fwd_pairs_tiles_bn_bwd_stats(const float* in, const float* W, const int* pair_in, const int* pair_cnt, const int* pair_pos,
                                         float* out, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int64_t live_tiles, int flags,
                                         void* ws, int64_t ws_bytes, float* stats, const float* bn_x, const float* mean,
                                         const float* var, const float* gamma, const float* beta, float eps, int act,
                                         const float* add, const float* bn_y, hipStream_t stream);

/* backward-weights of ME.MinkowskiConvolution (autograd of me_resnet.py:19-21, :56-62 and fcaf3d_neck_with_head.py:52,
 * :60-69; `gW[k] += in[i]^T (x) gout[o]`): gW[k] = sum_o in[nbr[k][o]]^T (x) gout[o];
 * deterministic two-level reduction.  FC_CONV_SPLIT (both entry points): the split kernels (csrc/wgrad_x6.h: fp32 in, fp32
 * accumulate, exact products) where one exists for the shape — dense tables that qualify for the multi-offset kernel, pair
 * lists, table-free GEMMs; the fp32 MFMA kernels otherwise. */
int64_t fc_conv_wgrad_ws_bytes(int64_t n_out, int K, int Cin, int Cout, int flags);
int fc_conv_wgrad(const float* in, const float* gout, const int* nbr, const int* row_index, float* gW, int64_t n_in,
                  int64_t n_out, int K, int Cin, int Cout, int flags, void* ws, int64_t ws_bytes, hipStream_t stream);
/* the same (autograd of me_resnet.py:56-62) over the exact pair lists of fc_kernel_map_pairs (Cin, Cout multiples of 64): the reduction skips absent
 * neighbours, which is ~40 % of a 27-offset table on surface-like scenes.  Workspace as fc_conv_wgrad_ws_bytes. */
int fc_conv_wgrad_pairs(const float* in, const float* gout, const int* pair_in, const int* pair_out, const int* pair_cnt,
                        float* gW, int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, void* ws,
                        int64_t ws_bytes, hipStream_t stream);

/* The stem convolution in training (me_resnet.py:19-21: `conv1` = ME.MinkowskiConvolution(3, 64, kernel_size=3, stride=2), K <= 27
 * offsets; its autograd for the weight): the forward additionally saves the gathered inputs of every output row as
 * col (n_out, 84) (27 x 3 floats, zero-padded), and the weight gradient gW (K,3,64) = col^T @ gout streams col and gout
 * instead of repeating 27 scattered 12-byte reads per output row.  col == NULL: plain forward (= fc_conv_fwd). */
int fc_stem_conv_fwd(const float* in, const float* W, const int* nbr, float* out, float* col, int64_t n_in, int64_t n_out,
                     int K, hipStream_t stream);
int64_t fc_stem_conv_wgrad_ws_bytes(int64_t n_out, int K);
int fc_stem_conv_wgrad(const float* col, const float* gout, float* gW, int64_t n_out, int K, void* ws, int64_t ws_bytes,
                       hipStream_t stream);

/* (K,Cin,Cout) -> (K,Cout,Cin): the W[k]^T of ME's backward-data rule `gin[i] += gout[o] @ W[k]^T` (SURVEY.md Appendix A.3;
 * autograd of me_resnet.py:56-62), so that the pass runs through fc_conv_fwd on the transposed table. */
int fc_transpose_weight(const float* W, float* Wt, int K, int Cin, int Cout, hipStream_t stream);

/* Which launch a convolution call becomes (No reference counterpart: ME chooses its kernels inside MinkowskiConvolution, the call
 * sites are me_resnet.py:56-62).  Pure host functions, no GPU needed: the route the entry points above compute before they launch
 * (csrc/conv_route.h), under the CURRENT fc_set_split_mode / fc_set_bf16_fast / fc_debug_set_h3r settings, written as 16 ints
 * (unused ones 0).  Return 0, or -1 exactly where the launch would (then out[0] = the INVALID family).
 * table_kind: FC_TABLE_* — none (nbr == NULL), a dense neighbour table, a table in sorted-row order (out_index), pair lists; for
 * fc_conv_fwd_route | FC_TABLE_STATS: the call asks for the statistics epilogue (fc_conv_fwd_stats and its kin), and live_tiles as
 * in fc_conv_fwd_pairs_tiles.  out[] of fc_conv_fwd_route, by FC_ROUTE_*: kernel family (FC_FAM_*), tile rows, tile columns, waves
 * along the rows, S = partial sums in the workspace (1: none), weight operand (FC_WSRC_*: fp32, fp32 read transposed, pre-split
 * image), arithmetic (FC_MODE_*: fp32, six bf16 products, bf16-fast, h3), buffer (1) / flat (0) addressing, where a statistics
 * epilogue runs (FC_EPI_*: not on this route, in the kernel, in the sum pass), the grid.  out[] of fc_conv_wgrad_route, by
 * FC_WROUTE_*: family (FC_WFAM_*), Cin tile, Cout tile, offsets per workgroup, rows per chunk, table kind, arithmetic, S = row
 * ranges, rows per range, buffer addressing, grid.y (grid.x = S). */
enum { FC_TABLE_NONE, FC_TABLE_DENSE, FC_TABLE_SORTED, FC_TABLE_PAIRS, FC_TABLE_STATS = 8 };
enum { FC_FAM_INVALID, FC_FAM_STEM, FC_FAM_FMA, FC_FAM_MFMA, FC_FAM_MFMA_P, FC_FAM_GLDS, FC_FAM_X6, FC_FAM_H3R };
enum { FC_WFAM_INVALID, FC_WFAM_STEM, FC_WFAM_FMA, FC_WFAM_MFMA, FC_WFAM_MFMA_P, FC_WFAM_MULTI, FC_WFAM_X6T };
enum { FC_WSRC_FP32, FC_WSRC_FP32_T, FC_WSRC_IMAGE };
enum { FC_MODE_FP32, FC_MODE_SIX, FC_MODE_BF16, FC_MODE_H3 };
enum { FC_EPI_NONE, FC_EPI_KERNEL, FC_EPI_SUM };
enum { FC_ROUTE_FAMILY, FC_ROUTE_BM, FC_ROUTE_BN, FC_ROUTE_WM, FC_ROUTE_S, FC_ROUTE_WSRC, FC_ROUTE_MODE, FC_ROUTE_BUF, FC_ROUTE_EPI,
       FC_ROUTE_GRID_X, FC_ROUTE_GRID_Y, FC_ROUTE_GRID_Z };
enum { FC_WROUTE_FAMILY, FC_WROUTE_BM, FC_WROUTE_BN, FC_WROUTE_KO, FC_WROUTE_BKR, FC_WROUTE_TABLE, FC_WROUTE_MODE, FC_WROUTE_S,
       FC_WROUTE_RPS, FC_WROUTE_WBUF, FC_WROUTE_GRID_Y };
int fc_conv_fwd_route(int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, int table_kind, int64_t live_tiles,
                      int* out);
int fc_conv_wgrad_route(int64_t n_in, int64_t n_out, int K, int Cin, int Cout, int flags, int table_kind, int* out);

/* ---- normalisation / pooling / rows ------------------------------------------------------- */

/* column statistics per segment: MinkowskiBatchNorm (seg == NULL, one segment: all voxels on this GPU)
 * and MinkowskiInstanceNorm (seg = &coords[0], seg_stride = 4: per scene) — me_resnet.py:22,63. */
int64_t fc_col_stats_ws_bytes(int64_t n, int C, int nseg);
int fc_col_stats(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* mean, float* var,
                 float* cnt, void* ws, int64_t ws_bytes, hipStream_t stream);

/* per-segment column sums (deterministic): the per-scene loss normalisers of fcaf3d_neck_with_head.py:178-187. */
int fc_seg_col_sums(const float* x, const int* seg, int seg_stride, int64_t n, int C, int nseg, float* out, void* ws,
                    int64_t ws_bytes, hipStream_t stream);
/* nn.BatchNorm1d training-mode buffer update inside ME.MinkowskiBatchNorm (momentum, unbiased variance) —
 * me_resnet.py:48-50, BasicBlock norm1/norm2, fcaf3d_neck_with_head.py:53, :62, :68. */
int fc_bn_running_update(const float* mean, const float* var, const float* cnt, float momentum, int C, float* running_mean,
                         float* running_var, long long* num_batches_tracked, hipStream_t stream);

/* y = act((x-mean)/sqrt(var+eps)*gamma + beta (+ residual)); act 0 none, 1 ReLU, 2 ELU —
 * ME.MinkowskiInstanceNorm + MinkowskiReLU of the stem (me_resnet.py:22-23), ME.MinkowskiBatchNorm + MinkowskiELU of the
 * neck (fcaf3d_neck_with_head.py:53-54, :62-63, :68-70), BasicBlock's norm / `out += residual` / relu (Appendix A.6, A.7);
 * fc_norm_act_bwd is their autograd. */
int fc_norm_act_fwd(const float* x, const int* seg, int seg_stride, int64_t n, int C, const float* mean, const float* var,
                    float eps, const float* gamma, const float* beta, const float* residual, int act, float* y,
                    hipStream_t stream);
int64_t fc_norm_act_bwd_ws_bytes(int64_t n, int C, int nseg);
int fc_norm_act_bwd(const float* x, const float* y, const float* gy, const int* seg, int seg_stride, int64_t n, int C,
                    int nseg, const float* mean, const float* var, const float* cnt, float eps, const float* gamma,
                    const float* beta, int act, float* gx, float* gres, float* sums, void* ws, int64_t ws_bytes,
                    hipStream_t stream);

/* Training-mode ME.MinkowskiBatchNorm (+ fused ReLU/ELU / residual; the BasicBlock norms of me_resnet.py:3, :56-63 and the
 * neck norms of fcaf3d_neck_with_head.py:53, :62, :68) for small feature matrices in TWO launches per direction: batch statistics, running-buffer update (nn.BatchNorm1d momentum / unbiased variance) and apply. */
int64_t fc_bn_stats_ws_bytes(int64_t n, int C);
int fc_bn_stats_train(const float* x, int64_t n, int C, float momentum, float* mean, float* var, float* cnt,
                      float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                      int64_t ws_bytes, hipStream_t stream);
int64_t fc_bn_small_ws_bytes(int C);
int fc_bn_act_train_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta,
                        const float* residual, int act, float momentum, float* y, float* mean, float* var, float* cnt,
                        float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                        int64_t ws_bytes, hipStream_t stream);
int fc_bn_act_train_bwd(const float* x, const float* y, const float* gy, int64_t n, int C, const float* mean,
                        const float* var, float eps, const float* gamma, const float* beta, int act, float* gx, float* gres,
                        float* sums, void* ws, int64_t ws_bytes, hipStream_t stream);

/* r5 — training-mode ME.MinkowskiBatchNorm (BasicBlock norm1 / norm2 / downsample norm: me_resnet.py:3, :56-63; the neck's
 * norms: fcaf3d_neck_with_head.py:53, :62, :68) as ONE entry point per direction for every matrix size, with the two fusions
 * the launch-list executor uses:
 *   forward, `part` != NULL: the batch statistics come from column sums the PRODUCER of x left in its epilogue
 *     (fc_conv_fwd_stats / fc_conv_fwd_pairs_tiles_stats: part[nb_part][2][groups * C] = sums of x and x^2 per row block; groups = 8
 *     for the (n, 8 C) GEMM of a generative transposed convolution viewed as (8 n, C)), combined in fp64 in a fixed order — no read
 *     pass over x for the statistics; nb_part <= 64: one launch (every block of the apply kernel re-reduces the table), else two;
 *   backward, `gy2` != NULL: a second contribution to the incoming gradient, added on the fly (a tensor with two consumers:
 *     BasicBlock's `out += residual`, me_resnet.py:3) instead of a separate add pass.
 * part == NULL / gy2 == NULL: exactly fc_bn_act_train_fwd/bwd (n * C <= small_elems) or fc_bn_stats_train + fc_norm_act_fwd /
 * fc_norm_act_bwd.  sums (2, C) = [d beta, d gamma]. */
int64_t fc_bn_train_ws_bytes(int64_t n, int C);
int fc_bn_train_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta, const float* residual,
                    int act, float momentum, float* y, float* mean, float* var, float* cnt, float* running_mean,
                    float* running_var, long long* num_batches_tracked, const float* part, int64_t nb_part, int groups,
                    int64_t small_elems, void* ws, int64_t ws_bytes, hipStream_t stream);
int fc_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gy2, int64_t n, int C, const float* mean,
                    const float* var, const float* cnt, float eps, const float* gamma, const float* beta, int act, float* gx,
                    float* gres, float* sums, const float* part, int64_t nb_part, int64_t small_elems, void* ws, int64_t ws_bytes,
                    hipStream_t stream);

/* Which launches a training-mode normalisation call becomes (fc_bn_train_fwd / _add_fwd and the backward entry points: ME.MinkowskiBatchNorm /
 * MinkowskiInstanceNorm with their activations, me_resnet.py:3, :22-23, :56-63; fcaf3d_neck_with_head.py:53, :62, :68).  Pure host
 * functions, no GPU needed: the route the entry points compute before they launch (csrc/norm_route.h), written as 16 ints (unused
 * ones 0).  Return 0, or -1 exactly where the entry point would for these sizes (then out[0] = 0, the INVALID family).
 * fc_bn_train_fwd_route: the arguments of fc_bn_train_fwd (fc_bn_act_train_fwd: small_elems = INT64_MAX; fc_bn_stats_train: the
 * statistics step of small_elems = -1).  fc_bn_train_bwd_route, form (FC_NFORM_*): TRAIN fc_bn_train_bwd, SMALL fc_bn_act_train_bwd,
 * SEG fc_norm_act_bwd and fc_maxpool8_norm_act_bwd (n = n_in); has_part / nb_part / small_elems as in fc_bn_train_bwd (TRAIN only).
 * out[] of both, by FC_NROUTE_*: who makes the per-block sums — forward, the batch statistics (FC_NSTATS_*: the apply kernel's
 * prologue over the producer's table, k_bn1_partial on <= 64 blocks, k_bn1_partial on <= 1024 blocks + k_bn_finalize,
 * k_bn2_finalize over the table); backward, the sums of g' and g' xhat (FC_NRED_*: the producer's table, k_norm_bwd_partial) —,
 * the apply step (forward FC_NAPPLY_*: k_bn1_apply, k_bn2_apply, k_norm_act_fwd; backward FC_NBAPPLY_*: none — no rows, sums
 * zero-filled —, k_bn1_bwd_apply re-reducing in its prologue, k_stats_final + k_norm_bwd_apply), where the word of fc_amax_out_hint
 * is filled (FC_NAMAX_*: by the apply kernel, by a pass of its own), the blocks of the table of sums, row blocks / rows per block /
 * channels per block of a prologue-reducing apply kernel, threads / LDS bytes / grid of the apply kernel, the workspace bytes the
 * entry point checks, the kernel launches (the amax pass not counted). */
enum { FC_NFORM_TRAIN, FC_NFORM_SMALL, FC_NFORM_SEG };
enum { FC_NSTATS_INVALID, FC_NSTATS_PROLOGUE, FC_NSTATS_PARTIAL_SMALL, FC_NSTATS_PARTIAL, FC_NSTATS_TABLE };
enum { FC_NAPPLY_NONE, FC_NAPPLY_BN1, FC_NAPPLY_BN2, FC_NAPPLY_ROWS };
enum { FC_NAMAX_NONE, FC_NAMAX_FOLDED, FC_NAMAX_PASS };
enum { FC_NRED_INVALID, FC_NRED_TABLE, FC_NRED_PARTIAL, FC_NRED_NONE };
enum { FC_NBAPPLY_NONE, FC_NBAPPLY_PROLOGUE, FC_NBAPPLY_FINAL, FC_NBAPPLY_ROWS };
enum { FC_NROUTE_SUMS, FC_NROUTE_APPLY, FC_NROUTE_AMAX, FC_NROUTE_NP, FC_NROUTE_NB, FC_NROUTE_RPB, FC_NROUTE_CG, FC_NROUTE_THREADS, FC_NROUTE_LDS,
       FC_NROUTE_GRID_X, FC_NROUTE_GRID_Y, FC_NROUTE_WS_BYTES, FC_NROUTE_LAUNCHES };
int fc_bn_train_fwd_route(int64_t n, int C, int has_part, int64_t nb_part, int groups, int64_t small_elems, int* out);
int fc_bn_train_bwd_route(int64_t n, int C, int nseg, int has_part, int64_t nb_part, int64_t small_elems, int form, int* out);

/* The backward through a BatchNorm in eval mode whose layer still trains (mmdet's norm_eval; ME.MinkowskiBatchNorm after .eval(),
 * me_resnet.py:3, :56-63; fcaf3d_neck_with_head.py:53, :62, :68): y = act(xhat gamma + beta (+ res)), xhat = (x - running_mean) rstd,
 * rstd = 1 / sqrt(running_var + eps), both statistics constants.  With g' = (gy (+ gy2)) act'(pre) — act' recomputed from x where y == NULL
 * (no residual in the forward), else read from y, as fc_bn_train_bwd —: gx = g' gamma rstd, gres = g' (nullable), sums (2, C) = [d beta =
 * sum g', d gamma = sum g' xhat].  gx depends on neither sum, so the rows are read ONCE, by one kernel.
 * sums == NULL (gamma and beta frozen): pure elementwise, one launch, no workspace.  sums != NULL: the same pass leaves per-row-block
 * partial sums in ws (fc_bn_eval_bwd_ws_bytes) and a second launch adds them in a fixed order — no float atomics, bit-reproducible.
 * amax_gx (nullable): max |gx| folded into the caller's zeroed FC_AMAX_SLOT_BYTES slot, for the convolution that gathers gx.
 * n == 0: FC_OK, sums zero-filled, nothing else launched.  n < 0, C < 4, C % 4, C > 1024, act outside 0..2: FC_EINVAL; a short workspace:
 * FC_EWS; nothing is launched on a refused call.  fc_bn_eval_bwd_route: the route as data, out[] as fc_bn_train_bwd_route (FC_NROUTE_*):
 * sums FC_NRED_PARTIAL or FC_NRED_NONE, apply FC_NBAPPLY_ROWS (FC_NBAPPLY_NONE: no rows), row blocks / rows per block of the row-blocked
 * pass, threads / LDS / grid of the kernel, the workspace bytes the entry point checks, the launches. */
int fc_bn_eval_bwd(const float* x, const float* y, const float* gy, const float* gy2, int64_t n, int C, const float* running_mean,
                   const float* running_var, float eps, const float* gamma, const float* beta, int act, float* gx, float* gres,
                   float* sums, unsigned* amax_gx, void* ws, int64_t ws_bytes, hipStream_t stream);
int64_t fc_bn_eval_bwd_ws_bytes(int64_t n, int C, int want_sums);
int fc_bn_eval_bwd_route(int64_t n, int C, int want_sums, int* out);

/* ME.MinkowskiMaxPooling(k=2,s=2) — me_resnet.py:24. */
int fc_maxpool_fwd(const float* in, const int* nbr, int64_t n_out, int K, int C, float* out, int* argrow,
                   hipStream_t stream);
int fc_maxpool_bwd(const float* gout, const int* argrow, int64_t n_out, int C, float* gin, hipStream_t stream);

/* r7 — the stem's tail, ME.MinkowskiInstanceNorm + MinkowskiReLU + MinkowskiMaxPooling(k=2,s=2) (me_resnet.py:22-24), without the
 * normalised tensor in between.  Forward: out / argrow (n_out, C) bit for bit those of fc_norm_act_fwd (no residual) followed by
 * fc_maxpool_fwd over the (8, n_out) child table nbr — the activation is applied before the comparison, the first maximum in
 * offset order wins ties, absent children are skipped, a row without children gives 0 / -1; y != NULL: the normalised rows are
 * stored as well (every child row once).  seg (stride seg_stride ints, NULL = one scene) is the scene of an INPUT row; the children
 * of a pooled row lie in one scene.  Folds max |out| into the word of fc_amax_out_hint.
 * parent != NULL: parent[child row] = pooled row is stored as well (n_in ints), for the backward pass.
 * Backward (the autograd of the pair): fc_norm_act_bwd (y == NULL, no residual) whose incoming gradient is read through the pool —
 * row r receives gout[parent[r]][c] where argrow[parent[r]][c] == r, else 0 — instead of from the matrix a zero fill + fc_maxpool_bwd
 * would write: the same launches, rows and summation order, so gx (n_in, C) and sums (nseg, 2, C) = [d beta, d gamma] per scene are bit
 * for bit those of the three operators.  seg = scene of an INPUT row; every input row must be the child of a pooled row (the rows of
 * a k2s2 stride map are): parent[] of any other row is not written. */
int fc_norm_act_maxpool8_fwd(const float* x, const int* seg, int seg_stride, int C, const float* mean, const float* var, float eps,
                             const float* gamma, const float* beta, int act, const int* nbr, int64_t n_out, float* out,
                             int* argrow, float* y, int* parent, hipStream_t stream);
int64_t fc_maxpool8_norm_act_bwd_ws_bytes(int64_t n_in, int C, int nseg);
int fc_maxpool8_norm_act_bwd(const float* x, const float* gout, const int* argrow, const int* parent, const int* seg, int seg_stride,
                             int64_t n_in, int C, int nseg, const float* mean, const float* var, const float* cnt, float eps,
                             const float* gamma, const float* beta, int act, float* gx, float* sums, void* ws, int64_t ws_bytes,
                             hipStream_t stream);

/* The same pair (me_resnet.py:22-24) with a per-child arg-max MASK between the directions instead of the arg-max rows: mask (n_in 64-bit
 * words, one per INPUT row r) has bit c set exactly where argrow[parent[r]][c] == r.  C must be 64 (anything else: -1); parent and mask are
 * required.  Forward: out, parent, y and the amax word are those of fc_norm_act_maxpool8_fwd; argrow may be NULL and is then not stored.
 * Backward: the launches, route (FC_NFORM_SEG over the n_in rows), workspace (fc_maxpool8_norm_act_bwd_ws_bytes) and summation order of
 * fc_maxpool8_norm_act_bwd, and `bit ? gout[parent[r]][c] : 0` has the values of its arg-max comparison: gx and sums are bit for bit
 * its.  Per input row the backward kernels read 8 linear bytes where they gathered 256 bytes of arg-max rows. */
int fc_norm_act_maxpool8_mask_fwd(const float* x, const int* seg, int seg_stride, int C, const float* mean, const float* var, float eps,
                                  const float* gamma, const float* beta, int act, const int* nbr, int64_t n_out, float* out,
                                  int* argrow, float* y, int* parent, unsigned long long* mask, hipStream_t stream);
int fc_maxpool8_mask_norm_act_bwd(const float* x, const float* gout, const unsigned long long* mask, const int* parent, const int* seg,
                                  int seg_stride, int64_t n_in, int C, int nseg, const float* mean, const float* var, const float* cnt,
                                  float eps, const float* gamma, const float* beta, int act, float* gx, float* sums, void* ws,
                                  int64_t ws_bytes, hipStream_t stream);

/* r7 — the neck's sparse sum `inputs[i] + x` (fcaf3d_neck_with_head.py:101) written by the normalisation that produces x: where
 * every row of inputs[i] lies in x's coordinate set the sum is x with inputs[i] added at rows[.].  fc_inverse_rows: inv (n_inv
 * ints) = -1, then inv[rows[i]] = i for i < n (rows unique).  fc_norm_act_add_fwd / fc_bn_train_add_fwd: fc_norm_act_fwd /
 * fc_bn_train_fwd with y[r] += add_src[add_inv[r]] where add_inv[r] >= 0, behind the activation (one fp32 add per element, the
 * one fc_scatter_rows_add performs: same bits), and max |y| of the SUM folded into the word of fc_amax_out_hint.  The layer's
 * backward must not read y (no residual: act' is recomputed from x).  add_inv == add_src == NULL: exactly the plain entry points. */
int fc_inverse_rows(const int* rows, int64_t n, int64_t n_inv, int* inv, hipStream_t stream);
int fc_norm_act_add_fwd(const float* x, const int* seg, int seg_stride, int64_t n, int C, const float* mean, const float* var,
                        float eps, const float* gamma, const float* beta, const float* residual, int act, const int* add_inv,
                        const float* add_src, float* y, hipStream_t stream);
int fc_bn_train_add_fwd(const float* x, int64_t n, int C, float eps, const float* gamma, const float* beta, const float* residual,
                        int act, float momentum, float* y, float* mean, float* var, float* cnt, float* running_mean,
                        float* running_var, long long* num_batches_tracked, const float* part, int64_t nb_part, int groups,
                        int64_t small_elems, const int* add_inv, const float* add_src, void* ws, int64_t ws_bytes,
                        hipStream_t stream);

/* feature rows of MinkowskiPruning (fcaf3d_neck_with_head.py:124-125), of the sparse sum `inputs[i] + x` (:101) and of
 * the per-scene decomposition (:266-275); fc_scatter_rows_add is the autograd of the gather. */
int fc_gather_rows(const float* src, const int* idx, int64_t n, int C, float* dst, hipStream_t stream);
int fc_scatter_rows_add(const float* src, const int* idx, int64_t n, int C, float* dst, hipStream_t stream);

/* ---- losses ------------------------------------------------------------------------------- */

/* mmcv sigmoid_focal_loss forward/backward (through mmdet FocalLoss, fcaf3d_neck_with_head.py:29-34,:180):
 * loss_rows[n] = row_weight[n] * sum_c loss[n,c] (row_weight nullable = 1); labels int64 in {-1,0..C-1},
 * -1 = background (all classes negative).  backward: glogits = dloss/dlogits * row_weight[n] * gscale_dev[0]. */
int fc_focal_loss_fwd(const float* logits, const long long* labels, const float* row_weight, int64_t n, int C, float gamma,
                      float alpha, float* loss_rows, hipStream_t stream);
int fc_focal_loss_bwd(const float* logits, const long long* labels, const float* row_weight, int64_t n, int C, float gamma,
                      float alpha, const float* gscale_dev, float* glogits, hipStream_t stream);

/* axis-aligned 3D IoU of (n,6) [cx,cy,cz,w,l,h] boxes and its gradient w.r.t. pred —
 * iou3d_loss.py:21-35 over iou3d_calculator.py:201-330 (is_aligned=True). dpred may be NULL. */
int fc_aiou3d_fwd_bwd(const float* pred, const float* target, int target_stride, int64_t n, float eps, float* iou,
                      float* dpred, hipStream_t stream);

/* Fcaf3DNeckWithHead._loss_single (fcaf3d_neck_with_head.py:160-203) for every location of the batch in one pass, yaw-less
 * heads: sigmoid focal loss (:180), BCE-with-logits centerness loss on the positives (:191-193) and the axis-aligned
 * IoU loss on _bbox_pred_to_bbox (:281-300; iou3d_loss.py:21-35), each row weighted by its scene's 1 / (B * normaliser)
 * (inv_pos, inv_den: (B,) device arrays; scene: (n) int32), summed deterministically and scaled by the loss weights.
 * labels int64 in {-1, 0..C-1}; bbox_t (n,7) gravity-centre targets.  Backward: gradients w.r.t. cls_score (n,C),
 * centerness (n), bbox_pred (n,6) for incoming scalar gradients g_* (device, NULL = loss unused). */
int64_t fc_fcaf3d_loss_ws_bytes(int64_t n);
int fc_fcaf3d_loss_fwd(const float* points, const float* bbox_pred, const float* centerness, const float* cls_score,
                       const float* centerness_t, const float* bbox_t, const long long* labels, const int* scene,
                       const float* inv_pos, const float* inv_den, int64_t n, int n_classes, float gamma, float alpha,
                       float lw_cls, float lw_centerness, float lw_bbox, float* loss_cls, float* loss_centerness,
                       float* loss_bbox, void* ws, int64_t ws_bytes, hipStream_t stream);
int fc_fcaf3d_loss_bwd(const float* points, const float* bbox_pred, const float* centerness, const float* cls_score,
                       const float* centerness_t, const float* bbox_t, const long long* labels, const int* scene,
                       const float* inv_pos, const float* inv_den, int64_t n, int n_classes, float gamma, float alpha,
                       float lw_cls, float lw_centerness, float lw_bbox, const float* g_cls, const float* g_centerness,
                       const float* g_bbox, float* grad_cls_score, float* grad_centerness, float* grad_bbox_pred,
                       hipStream_t stream);

/* rotated 3D IoU of (n,7) [cx,cy,cz,w,l,h,yaw] boxes and its gradient w.r.t. pred — cal_iou_3d,
 * rotated_iou/oriented_iou_loss.py:86-109 + box_intersection_2d.py:13-184 + cuda_op sort_v.
 * weight (nullable): rows with weight <= 0 are skipped (iou = 0, dpred = 0). */
int fc_riou3d_fwd_bwd(const float* pred, const float* target, const float* weight, int64_t n, float* iou, float* dpred,
                      hipStream_t stream);

/* `kind` of fc_eiou3d_fwd_bwd */
enum { FC_EIOU_GIOU = 0, FC_EIOU_DIOU = 1 };
/* The enclosing-box losses and their gradient w.r.t. pred, fused — oriented_iou_loss.py:112-152 (cal_giou_3d, cal_diou_3d),
 * min_enclosing_box.py:142-172 (smallest_bounding_box), iou3d_calculator.py:290-319 (axis-aligned giou; the aligned DIoU has no
 * reference function: cal_diou_3d(enclosing_type='aligned') at yaw 0).  box_dim 7: rows [cx,cy,cz,w,l,h,yaw]; box_dim 6: axis-aligned
 * rows; target rows are target_stride >= box_dim floats apart.  Outputs: loss (n), iou (n), dpred (n, box_dim) = d loss[i] / d pred[i].
 * weight (nullable): a row with !(weight[i] > 0) gets loss = iou = 0 and a zero dpred row, and its boxes are not read (they may
 * hold NaN or inf).  The extent along a candidate line uses the line's unit direction instead of the reference's slope
 * (DESIGN.md section 16).  Pairs whose enclosing box has no extent give NaN / inf as in the reference.  n == 0: FC_OK, nothing
 * launched; n < 0, another box_dim or kind: FC_EINVAL. */
int fc_eiou3d_fwd_bwd(const float* pred, const float* target, int target_stride, const float* weight, int64_t n, int box_dim,
                      int kind, float* loss, float* iou, float* dpred, hipStream_t stream);

/* Epilogue of Fcaf3DNeckWithHead.forward_single (fcaf3d_neck_with_head.py:256-279) on the output y (n, ld <= 64) of the
 * fused 1x1 head GEMM, columns [centerness | reg (n_reg = 6 or 8) | cls (n_cls) | padding]:
 *   centerness (n,1) = y[:,0];  bbox_pred (n,n_reg) = [exp(scale * reg[:, :6]) | reg[:, 6:]];
 *   cls_score (n,n_cls) = y[:, 1+n_reg:] + bias;  cls_max (n) = max_c cls_score (the score `_prune` interpolates, :117-121).
 * bwd: gy (n, ld) from the three output gradients (any may be NULL = zero), gscale_row (n) = per-row d/dscale. */
int fc_head_split_fwd(const float* y, int ld, const float* bias, const float* scale_dev, int64_t n, int n_reg, int n_cls,
                      float* centerness, float* bbox_pred, float* cls_score, float* cls_max, hipStream_t stream);
int fc_head_split_bwd(const float* y, int ld, const float* scale_dev, const float* bbox_pred, const float* g_centerness,
                      const float* g_bbox, const float* g_cls, int64_t n, int n_reg, int n_cls, float* gy,
                      float* gscale_row, hipStream_t stream);
/* fc_head_split_bwd plus, in the same pass, the two reductions autograd would run over its outputs: gbias (n_cls) = column sums
 * of g_cls — the gradient of cls_conv's bias (fcaf3d_neck_with_head.py:262, init :91-92) — and gscale (1) = sum of the per-row
 * d/dscale terms — the gradient of Scale.scale (:273-275); either may be NULL.  Two launches (64 rows per workgroup leave
 * 65 partial sums each in ws; one 1024-thread block per column adds them in a fixed order). */
int64_t fc_head_split_bwd_sums_ws_bytes(int64_t n);
int fc_head_split_bwd_sums(const float* y, int ld, const float* scale_dev, const float* bbox_pred, const float* g_centerness,
                           const float* g_bbox, const float* g_cls, int64_t n, int n_reg, int n_cls, float* gy, float* gbias,
                           float* gscale, void* ws, int64_t ws_bytes, hipStream_t stream);

/* `cuda_ext.sort_v(vertices, mask, num_valid)` of the un-vendored Rotated_IoU extension (docker/Dockerfile:35-40),
 * bound by the reference at rotated_iou/box_intersection_2d.py:147: vertices (n_pairs,24,2) f32 centred on the mean
 * of the valid ones, mask (n_pairs,24) bool bytes, num_valid (n_pairs) i32 -> idx (n_pairs,9) i32: valid vertices in
 * angular order, closed (idx[nv] = idx[0]), padded with the first masked intersection slot.
 * fc_riou3d_fwd_bwd has this step fused in; this entry point is the drop-in for the Python-level op. */
int fc_sort_v(const float* vertices, const unsigned char* mask, const int* num_valid, int64_t n_pairs, int* idx,
              hipStream_t stream);

/* Fcaf3DAssigner.assign + compute_centerness (fcaf3d_neck_with_head.py:377-384, :394-466) for ALL scenes of the
 * batch: points (N,3) = locations of every level and scene; scene/level (N) ids; boxes (B,M,7) gravity-centre GT
 * boxes padded to M per scene, box_count (B); order (N) = rows grouped by (level, scene), seg_start (L*B+1).
 * Outputs per location: centerness target (0 for background), box target (7), label (-1 = background). */
int64_t fc_assign_ws_bytes(int B, int M, int L);
int fc_assign_targets(const float* points, const int* scene, const int* level, int64_t N, const float* boxes,
                      const long long* labels, const int* box_count, int B, int M, int L, const int* order,
                      const int* seg_start, int limit, int topk, float* centerness_t, float* bbox_t, long long* labels_out,
                      void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- NMS ---------------------------------------------------------------------------------- */

/* pcdet_nms nms_gpu (rotated=1) / nms_normal_gpu (rotated=0) — iou3d_nms.cpp:90-186, kernels
 * iou3d_nms_kernel.cu:267-372 — for `nseg` classes at once: boxes (nseg,stride,7) sorted by descending
 * score inside each segment, counts_dev (nseg) valid boxes per segment; keep (nseg,stride) receives the
 * ascending positions of the survivors, keep_count (nseg) their number.  Greedy scan runs on the device. */
int64_t fc_nms_bev_ws_bytes(int nseg, int stride);
int fc_nms_bev(const float* boxes, const int* counts_dev, int nseg, int stride, float thresh, int rotated,
               unsigned long long* mask_ws, int64_t ws_bytes, int* keep, int* keep_count, hipStream_t stream);
/* pcdet_nms boxes_iou_bev_gpu (iou3d_nms_kernel.cu:251-265): (n,m) BEV IoU matrix. */
int fc_boxes_iou_bev(const float* boxes_a, int n, const float* boxes_b, int m, int rotated, float* out,
                     hipStream_t stream);

/* ---- test-time augmentation merge (fcaf3d_amd/csrc_post/merge.hip) ------------------------------------------------ */

/* `flags` of fc_merge_sorted_segments: FC_MERGE_TO_BOTTOM converts gravity-centre input boxes to the bottom-centre tensor of
 * DepthInstance3DBoxes first (base_box3d.py:62-66); FC_MERGE_WITH_YAW lets the flips touch the yaw column (depth_box3d.py:189-197).
 * Bits of a segment descriptor's word [3] above its fp32 scale: the flips of that input segment. */
#define FC_MERGE_TO_BOTTOM 1
#define FC_MERGE_WITH_YAW 2
#define FC_MERGE_XF_FLIP_H (1ull << 32)
#define FC_MERGE_XF_FLIP_V (1ull << 33)
/* merge_aug_bboxes_3d (mmdet3d/core/post_processing/merge_augs.py:36-47, the concatenation of the mapped-back results of every
 * augmentation in augmentation order, and :65-89, the class-major lists sorted by descending score and cut to max_num) as a
 * stable k-way merge: output segment o takes the input segments g = o*K + k, k = 0..K-1, each sorted by descending score.
 * desc (nseg_out*K, 4) int64 per input segment: [0] row r of counts_dev / keep / ord it reads, [1] box row base, [2] score
 * element base, [3] transform = fp32 bit pattern of the scale (bits 0-31) | FC_MERGE_XF_FLIP_H | FC_MERGE_XF_FLIP_V.  Element p
 * of segment g (p < counts_dev[r]) is table row t = ord[r*ord_stride + keep[r*keep_stride + p]] (keep / ord nullable: identity),
 * its score scores[desc[2] + t*score_stride], its box boxes[(desc[1] + t)*7 .. +7], mapped back as bbox3d_mapping_back
 * (core/bbox/transforms.py:4-23): flip horizontal, flip vertical, then the first six columns times the scale.  The result is
 * exactly `cat` in input-segment order + sort(descending=True, stable=True) + the first min(cap, stride_out) rows (cap < 0: no
 * cap): out_boxes (nseg_out, stride_out, 7), out_scores (nseg_out, stride_out), out_src (nseg_out, stride_out, 2) = (k, p)
 * (nullable), out_count (nseg_out) int32.  max_total: a host bound of the elements of any output segment (sizes the grid and
 * the workspace; elements beyond it are dropped).  No atomics: deterministic.  K <= 4096. */
int64_t fc_merge_sorted_segments_ws_bytes(int nseg_out, int max_total);
int fc_merge_sorted_segments(const int64_t* desc, int nseg_out, int K, const int* counts_dev, const int* keep, int keep_stride,
                             const int64_t* ord, int ord_stride, const float* scores, int score_stride, const float* boxes,
                             int flags, int max_total, int cap, float* out_boxes, float* out_scores, int* out_src,
                             int* out_count, int stride_out, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- test-time augmentation: box voting (fcaf3d_amd/csrc_post/vote.hip) -------------------------------------------------- */

/* `flags` of fc_vote_boxes: FC_VOTE_ROTATED takes the rotated BEV IoU (as fc_nms_bev with rotated = 1; otherwise the axis-aligned
 * one), FC_VOTE_WITH_YAW lets a member whose yaw differs from the kept box's by about a quarter turn vote with its sides exchanged. */
#define FC_VOTE_ROTATED 1
#define FC_VOTE_WITH_YAW 2
/* No reference counterpart (merge_aug_bboxes_3d keeps the NMS survivors as they are): box voting on the tables of fc_nms_bev.
 * boxes (nseg, stride, 7) and scores (nseg, stride), segment s holding counts_dev[s] <= max_count <= stride rows by descending
 * score; keep (nseg, keep_stride) the ascending kept positions fc_nms_bev wrote, keep_counts_dev[s] <= max_keep <= keep_stride of
 * them (max_count / max_keep: host bounds, larger device counts are cut to them; max_keep sizes the grid).  For every kept
 * position i of segment s the members are M = {i} and every j != i, j < count, with iou(i, j) >= vote_thr — the fp32 BEV IoU of
 * the NMS with a = box i, b = box j; a NaN is not a member — and
 *   out[i][k] = fp32( sum_{j in M} score_j * box_j[k] / sum_{j in M} score_j ), k = 0..5, both sums in fp64 over ascending j;
 *   out[i][6] = boxes[i][6].
 * FC_VOTE_WITH_YAW: d = remainder(yaw_j - yaw_i, fp32 pi); |d| > pi / 4: member j contributes (box_j[4], box_j[3]) to columns
 * (3, 4).  A weight sum that is not positive and finite leaves box i unchanged.  Rows that are not kept are copied to out_boxes
 * (nseg, stride, 7); rows at or past counts_dev[s] are neither read nor written; out_boxes must not alias boxes.  out_members
 * (nseg, keep_stride) int32, nullable: |M| per kept position.  0 < vote_thr <= 1.  One launch, no atomics: deterministic.
 * nseg == 0 or max_count == 0 launches nothing. */
int fc_vote_boxes(const float* boxes, const float* scores, const int* counts_dev, int nseg, int stride, int max_count,
                  const int* keep, const int* keep_counts_dev, int keep_stride, int max_keep, float vote_thr, int flags,
                  float* out_boxes, int* out_members, hipStream_t stream);

/* ---- evaluation: detection-to-ground-truth matching (fcaf3d_amd/csrc_post/eval.hip) ----------------------------------- */

/* `flags` of fc_eval_match: the detection boxes are the bottom-centre tensor of DepthInstance3DBoxes (what get_bboxes returns);
 * z += dz * 0.5 first, the gravity centre indoor_eval takes its IoU on. */
#define FC_EVAL_DET_BOTTOM 1
/* The matching of eval_det_cls (mmdet3d/core/evaluation/indoor_eval.py:86-146) for every scene and class of a set in one call.
 * det_boxes (n_det, det_dim) with det_dim 6 (yaw 0) or 7, det_scores (n_det) finite fp32, det_labels (n_det) int64; gt_boxes
 * (n_gt, 7) gravity centre, gt_labels (n_gt) int32; seg (n_scenes, 4) int64 (device) per scene: det_start, det_count, gt_start,
 * gt_count — the caller checks that the ranges lie inside [0, n_det) / [0, n_gt) and do not overlap; thr: n_thr <= 8 IoU
 * thresholds, fp64, on the device.  Per detection d of a scene, with label c:
 *   best_gt[d]  = index WITHIN THE SCENE's ground-truth range of the first maximum, in scene order, of the 3D IoU over the
 *                 scene's boxes of class c (the strict '>' scan of :131-136); -1 when the scene has no box of class c
 *   best_iou[d] = that IoU (rotated BEV overlap x height overlap / clamped 3D union, the fp32 value of nms.boxes_iou3d_gpu);
 *                 -inf when the scene has no box of class c
 *   tp_bits[d]  bit t: (double)best_iou > thr[t] and d is, among the scene's detections with the same best_gt that pass the same
 *                 test, the one with the highest score (equal scores: the lowest position in the scene) — the detection the
 *                 reference's walk in descending confidence reaches first (:138-146).
 * Detections outside every range get (-inf, -1, 0).  Any det_count / gt_count, zero included.  The winner is an unsigned 64-bit
 * minimum per (ground-truth box, threshold) in the workspace: deterministic.  n_det == 0 launches nothing. */
int64_t fc_eval_match_ws_bytes(int64_t n_det, int64_t n_gt, int n_thr);
int fc_eval_match(const float* det_boxes, int det_dim /* 6 or 7 */, const float* det_scores, const int64_t* det_labels,
                  const float* gt_boxes /* (n_gt,7) gravity centre */, const int* gt_labels,
                  const int64_t* seg /* (n_scenes,4): det_start, det_count, gt_start, gt_count */, int n_scenes,
                  int64_t n_det, int64_t n_gt, const double* thr /* device, n_thr <= 8 */, int n_thr, int flags,
                  float* best_iou, int* best_gt, unsigned char* tp_bits, void* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- optimizer (the reference's recipe, configs/fcaf3d/fcaf3d.py:30-31) --------------------------------- */

/* mmcv OptimizerHook grad_clip = dict(max_norm=10, norm_type=2) (configs/fcaf3d/fcaf3d.py:31; torch.nn.utils.clip_grad_norm_)
 * over ONE flat gradient buffer of n floats (n % 4 == 0; padding zero): out[0] = the global 2-norm, out[1] = the clip
 * coefficient min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0).  Nothing is scaled here: fc_adamw_step applies
 * the coefficient while it reads the gradient.  Deterministic two-level reduction. */
int64_t fc_grad_norm_ws_bytes(int64_t n);
int fc_grad_norm(const float* g, int64_t n, float max_norm, float* out, void* ws, int64_t ws_bytes, hipStream_t stream);
/* torch.optim.AdamW.step for optimizer = dict(type='AdamW', lr=0.001, weight_decay=0.0001) (configs/fcaf3d/fcaf3d.py:30)
 * over flat parameter / gradient / moment buffers (n % 4 == 0): decoupled weight decay, bias corrections
 * 1 - beta^step computed by the caller, gradient scaled by norm_and_clip[1] (device, nullable: the output of
 * fc_grad_norm).  One pass: 16 B read + 12 B written per parameter. */
int fc_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float bias_correction1, float bias_correction2, const float* norm_and_clip,
                  hipStream_t stream);

/* AdamW with a learning-rate and a weight-decay multiplier per parameter: optimizer = dict(type='AdamW', lr=0.001,
 * weight_decay=0.0001) (configs/fcaf3d/fcaf3d.py:30) with mmcv's paramwise_cfg on top.  mmcv's DefaultOptimizerConstructor is
 * third party and no config of the tree passes a paramwise_cfg: No reference counterpart for the constructor; the rule is restated
 * at runner.param_multipliers.  A RUN is a maximal stretch of consecutive parameters of the flat buffers with equal multipliers,
 * given by the float offset of its first parameter.  fc_adamw_groups_pack (pure host function) validates R runs over buffers of n
 * floats and packs them into `out` (fc_adamw_groups_table_bytes(R) bytes = 12 R; 0 for an R outside 1 .. FC_ADAMW_MAX_RUNS: R first
 * 64-float slice indices, R rate multipliers, R decay multipliers), which the caller uploads once.  FC_EINVAL: begin[0] != 0,
 * offsets not strictly ascending, an offset that is no multiple of 64 floats or is >= n, R < 1 or R > FC_ADAMW_MAX_RUNS, a
 * multiplier that is negative or not finite, n % 4 != 0, n / 64 >= 2^32; FC_EWS: out_bytes too small. */
#define FC_ADAMW_MAX_RUNS 1024
int64_t fc_adamw_groups_table_bytes(int R);
int fc_adamw_groups_pack(const int64_t* begin, const float* lr_mult, const float* decay_mult, int R, int64_t n, void* out,
                         int64_t out_bytes);
/* fc_adamw_step's pass (configs/fcaf3d/fcaf3d.py:30; same arithmetic, same 28 B per parameter, one launch) with lr * lr_mult[r]
 * and weight_decay * decay_mult[r] for the run r a 16-byte vector lies in; table_dev: the packed table of fc_adamw_groups_pack on
 * the device.  lr_mult == 0 leaves the run's parameters bit-unchanged while its moments advance; padding floats stay zero.  With
 * every multiplier 1 the result is fc_adamw_step's (the host calls that one then).  No reference counterpart for the run lookup. */
int fc_adamw_step_groups(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float bias_correction1, float bias_correction2, const float* norm_and_clip,
                         const void* table_dev, int R, hipStream_t stream);

/* mmcv EMAHook(momentum, interval, warm_up) (custom_hooks; mmcv/runner/hooks/ema.py of mmcv 1.3.x, third party and in no file of
 * the tree: No reference counterpart; the rule is restated at runner.WeightEma) riding in the optimizer's launch:
 * fc_adamw_step_groups' pass over p, g, m, v, and for every element, with p_new the parameter just computed,
 *     ema <- fl32( fl32(ema * ema_keep) + fl32(ema_mu * p_new) )          (three fp32 roundings, no fused multiply-add)
 * in the same thread: 36 B per parameter, one launch.  `ema`: n floats laid out like p (padding stays zero).  The caller forms
 * ema_keep = fl32(1 - mu) and calls this entry only on steps whose update is due.  table_dev == NULL with R == 0: no multipliers,
 * p / m / v come out as fc_adamw_step's; otherwise table_dev is the packed table of fc_adamw_groups_pack on the device and they
 * come out as fc_adamw_step_groups'.  FC_EINVAL: what fc_adamw_step_groups refuses (a table without 1 .. FC_ADAMW_MAX_RUNS runs, or
 * runs without a table), a null `ema` with n > 0, ema_mu or ema_keep outside [0, 1] or not finite. */
int fc_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bias_correction1, float bias_correction2, const float* norm_and_clip,
                      const void* table_dev, int R, float ema_mu, float ema_keep, hipStream_t stream);
/* mmcv EMAHook's exchange of the parameters and their averages at the epoch edges (after_train_epoch / before_train_epoch):
 * No reference counterpart in the tree.  a <-> b over n floats (n % 4 == 0) in 16-byte vectors, one launch, none for n == 0.
 * FC_EINVAL: a == b, overlapping ranges, a null pointer with n > 0, n < 0, n % 4 != 0. */
int fc_swap_f32(float* a, float* b, int64_t n, hipStream_t stream);

/* mmcv GradientCumulativeOptimizerHook(cumulative_iters=k) (optimizer_config; mmcv/runner/hooks/optimizer.py of mmcv 1.3.x, third
 * party and in no file of the tree: No reference counterpart; the rule is restated at runner.TrainStep) for a micro-iteration that
 * does NOT step, over flat buffers of n floats (n % 4 == 0): with scale = fl32(1 / factor),
 *     first != 0:  acc <- fl32(g * scale)                      (acc is not read: 8 B per parameter)
 *     first == 0:  acc <- fl32( acc + fl32(g * scale) )        (two fp32 roundings, no fused multiply-add: 12 B per parameter)
 * g is not written; padding that is zero in g stays zero in acc.  `ema` (nullable) with `p`: mmcv EMAHook's update falls due on
 * this iteration although the parameters did not move, and rides in the launch: ema <- fl32( fl32(ema * ema_keep) +
 * fl32(ema_mu * p) ) as in fc_adamw_ema_step, + 12 B per parameter.  One launch, none for n == 0.  FC_EINVAL: n < 0, n % 4 != 0,
 * a scale that is not finite or not positive, ema_mu or ema_keep outside [0, 1] or not finite (pass 0 without `ema`), `ema` without
 * `p`, a null acc or g with n > 0, acc overlapping g, ema overlapping acc, g or p. */
int fc_grad_accum(float* acc, const float* g, int64_t n, float scale, int first, float* ema, const float* p, float ema_mu,
                  float ema_keep, hipStream_t stream);
/* The STEPPING iteration of a group of more than one micro-iteration (mmcv GradientCumulativeOptimizerHook with grad_clip,
 * configs/fcaf3d/fcaf3d.py:31 for the clip): g_inout <- G = fl32( acc + fl32(g_inout * scale) ), the group's gradient, and in the
 * same pass out2 = [the global 2-norm of G, min(1, max_norm / (norm + 1e-6))] — bit for bit what fc_grad_norm returns for the
 * materialised G (its block assignment and order), so the pair of launches REPLACES fc_grad_norm (12 B per parameter instead of
 * 4; G is not re-read) and fc_adamw_step / fc_adamw_step_groups / fc_adamw_ema_step follows unchanged.  acc is not written.
 * out2 == NULL: the sum only, one launch, ws not used.  n == 0: nothing is launched and out2 is not written.  FC_EINVAL: n < 0,
 * n % 4 != 0, a scale that is not finite or not positive, a null buffer with n > 0, acc overlapping g_inout; FC_EWS: ws null or
 * smaller than fc_grad_accum_norm_ws_bytes(n) with out2 given. */
int64_t fc_grad_accum_norm_ws_bytes(int64_t n);
int fc_grad_accum_norm(float* g_inout, const float* acc, int64_t n, float scale, float max_norm, float* out2, void* ws,
                       int64_t ws_bytes, hipStream_t stream);

/* SURVEY.md 8(f) rank 4 "bf16 fast mode" (No reference counterpart: the reference trains in fp32 throughout, configs/fcaf3d/fcaf3d.py:30-33
 * sets no fp16 hook).  A process-global, flagged NON-PARITY switch: while on, the split-bf16 convolution launches that read a
 * weight image (FC_CONV_SPLIT | FC_CONV_IMAGE, 128-row tiles) and the split-bf16 weight-gradient launches multiply ONLY the leading bf16
 * piece of either operand (the operand rounded to nearest bf16; fp32 accumulate) — one MFMA product instead of six.  Default
 * off; `bench.py` reports it as `config.bf16_fast_mode` with "parity": false, never as `value`. */
int fc_set_bf16_fast(int on);

/* r6: the operand split of the matrix-pipe convolutions (No reference counterpart: MinkowskiEngine multiplies in fp32 FMA, the
 * call sites are mmdet3d/models/backbones/me_resnet.py:56-62 and every ME.MinkowskiConvolution of fcaf3d_neck_with_head.py:49-71).
 * mode 2 (default): every fp32 operand as TWO fp16 pieces, scaled by a power of two taken from the operand tensor's max |x|,
 * three exact products per fp32 product (csrc/conv_x6.h "h3": what is dropped is <= 2^-21 |a b| per product, 2^-25 on average
 * and unbiased — reductions measure closer to fp64 than an fp32 FMA chain); mode 0: three bf16 pieces, six products (r3-r5).  Process-global; weight images are built in the current mode and
 * must be read in it (rebuild them after a switch).  fc_get_split_mode: the mode launches use right now (0 while the bf16 fast
 * mode is on). */
int fc_set_split_mode(int mode);
int fc_get_split_mode(void);
/* max |x| over n floats (x 16-byte aligned) as a bit pattern -> slot[0]; slot = FC_AMAX_SLOT_BYTES (2 048) zero-initialised bytes
 * owned by the caller: 32 sub-words at a 64-byte stride whose MAXIMUM is the operand's amax (producers spread their folds over
 * them, fc_amax_out_hint); this pass writes sub-word 0, slot[1..2] are its scratch and return to zero.  Integer atomicMax: order-independent, bit-reproducible.  The mode-2 launches need
 * this word for their gathered operand(s); No reference counterpart (part of the operand split above, me_resnet.py:56-62). */
int fc_amax(const float* x, int64_t n, unsigned* slot, hipStream_t stream);
/* Hands the amax slots (device addresses; an UPPER bound of max |x| is enough) of the operands of the NEXT
 * fc_conv_fwd* / fc_conv_wgrad* call of the calling thread: amax_in for `in`, amax_gout for `gout` (weight gradients); NULL = the
 * library computes it itself with one fc_amax pass over the operand (a library-owned slot).  Cleared when that call returns.
 * No reference counterpart (see fc_set_split_mode; me_resnet.py:56-62). */
int fc_conv_amax_hint(const unsigned* amax_in, const unsigned* amax_gout);
/* The other end of the same word: the NEXT fc_bn_train_fwd / fc_bn_train_bwd / fc_norm_act_fwd / fc_norm_act_bwd / fc_bn_act_train_bwd /
 * fc_maxpool_fwd / fc_head_split_bwd_sums call of the calling thread also folds max |.| of what it writes (y, gx, out) into the slot at amax_word — one the
 * caller has ZEROED — from inside its apply kernel (one integer atomicMax per block), so that the convolution gathering that tensor
 * needs no fc_amax pass.  Cleared by that call.  No reference counterpart (see fc_set_split_mode; the producers are
 * ME.MinkowskiBatchNorm / MinkowskiReLU / MinkowskiELU / MinkowskiMaxPooling of me_resnet.py:19-24, fcaf3d_neck_with_head.py:49-71). */
int fc_amax_out_hint(unsigned* amax_word);
/* A/B switch (No reference counterpart; tests and tools/nbench): which mode-2 convolution launches on 128-row tiles run the
 * register-operand kernel csrc/conv_h3r.h — 0 none, 1 those on 128-column tiles (default), 2 all.  Results are bit-identical either
 * way (the statistics tables agree to rounding: other summation order). */
int fc_debug_set_h3r(int mode);

/* ---- launch-list executor (the network body in one call per direction) ------------------------------------ */

/* SingleStageSparse3DDetector.extract_feat (mmdet3d/models/detectors/single_stage_sparse.py:43-50: backbone me_resnet.py:43-50 +
 * Fcaf3DNeckWithHead.forward, fcaf3d_neck_with_head.py:94-108) and torch.autograd's backward over it, as a STATIC list of
 * operators walked natively: every operator is one of the entry points above with operands taken from host tables of device
 * addresses (`addr`), row counts (`dims`) and kernel-map descriptors (`maps`, fc_exec_map_words() int64 each) that the caller
 * refreshes per step; `ops` holds fc_exec_op_words() int64 per operator (layouts: fcaf3d_amd/csrc/exec_ops.h).
 * Operators [op_begin, op_end) run on streams[0] (caller's), streams[1] (head branch of the neck), streams[2] (weight
 * gradients), ordered by library-owned events.  ws / ws_bytes: one scratch buffer per stream; a sizing pass runs first: if a
 * buffer is too small NOTHING is launched, ws_need[3] receives the sizes and the call returns -2.
 * cfg[0]: the two-launch BatchNorm is used up to this many elements; cfg[1]: kernel-variant flags (the FC_CONV_* bits);
 * cfg[2] != 0: bracket every convolution operator with a HIP-event pair on its stream — fc_exec_probe_read(ms, meta, cap), called
 * after the device has drained, returns the number of brackets since the last read-out and writes their durations (ms) and
 * {map index | -1, direction, n_in, n_out, K, Cin, Cout, pair-list route} (8 int64 each): bench.py's live roofline measurement
 * (the reference times whole iterations only: tools/analysis_tools/benchmark.py:64-91).
 * cfg[3] != 0: the sizing pass only (ws_need is filled; 0 or -2; nothing is launched).  Events are kept per device; one caller
 * thread per device at a time. */
int fc_exec_op_words(void);
int64_t fc_exec_probe_read(float* ms, int64_t* meta, int64_t cap);
int fc_exec_map_words(void);
int fc_exec(const int64_t* ops, int64_t op_begin, int64_t op_end, const int64_t* addr, const int64_t* dims, const int64_t* maps,
            const int64_t* streams, const int64_t* ws, const int64_t* ws_bytes, int64_t* ws_need, const int64_t* cfg);

#ifdef __cplusplus
}
#endif
#endif /* FCAF3D_HIP_H */
