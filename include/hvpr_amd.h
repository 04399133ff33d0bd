/*
 * hvpr_amd — C-ABI of the MI355X (gfx950) hot path of HVPR's voxel-point encoding + BEV detection.
 *
 * Every entry point
 *   - takes plain device pointers + sizes and a stream (hipStream_t passed as void*); no torch types;
 *   - enqueues on that stream and returns without synchronising;
 *   - never allocates, frees or retains memory: inputs, outputs and workspaces are the caller's
 *     (sizes from the matching *_workspace_bytes function);
 *   - returns 0 on success, a negative hvpr_status otherwise (see hvpr_status_string); nothing throws.
 *   - data-dependent sizes (voxel counts, NMS keep counts) are written to device int32 words.
 *
 * Each function cites the reference interface it replaces (paths relative to the reference repo
 * cvlab-yonsei/HVPR).  The reference's own native boundary for these was three pybind11 torch
 * extensions built by setup.py:52-110 (iou3d_nms_cuda, pointnet2_batch_cuda, pointnet2_stack_cuda)
 * plus the external spconv voxel generator; their sources are not part of the reference snapshot.
 */
#ifndef HVPR_AMD_H
#define HVPR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *hvpr_stream_t; /* hipStream_t */

enum hvpr_status {
    HVPR_OK = 0,
    HVPR_ERR_INVALID_ARG = -1,   /* null pointer, negative size, inconsistent dims            */
    HVPR_ERR_UNSUPPORTED = -2,   /* a shape the kernels are not built for (documented per op) */
    HVPR_ERR_WORKSPACE = -3,     /* workspace too small                                        */
    HVPR_ERR_LAUNCH = -4,        /* hipGetLastError() != hipSuccess after the launch           */
    HVPR_ERR_TIMEOUT = -5        /* hvpr_voxelize_workspace_status: a one-launch index kernel gave up a wait (workspace needs a reset) */
};

int hvpr_abi_version(void);     /* 8 (history: csrc/abi.hip); size every workspace / packed buffer with the *_bytes / *_floats functions */
const char *hvpr_status_string(int status);

/* SyncBatchNorm across ranks (reference: tools/train.py:119-120, --sync_bn -> torch.nn.SyncBatchNorm).  The training entry points
 * that hold a whole BatchNorm inside ONE call — hvpr_pillar_vfe_train_fwd_f32 / hvpr_pillar_vfe_bwd_f32 (two BatchNorm1d) and
 * hvpr_spatial_gate_train_fwd_f32 / _bwd_f32 (one BatchNorm2d) — hand their per-rank sums to this hook between two of their
 * launches: fn must replace buf[0..n) (device doubles; buf[0] is the element count, then sum x, sum x^2 forward or sum dy,
 * sum dy xhat backward) by the sum over all ranks, enqueued so that work submitted to `stream` afterwards sees the result; it
 * returns 0 on success (anything else makes the entry point return HVPR_ERR_LAUNCH).  With the hook set the statistics, and the
 * input gradient, are those of the global batch; parameter gradients stay per-rank sums (the data-parallel wrapper reduces them),
 * as in torch.nn.SyncBatchNorm.  fn == NULL (the default) restores per-rank statistics.  This one pointer pair is the only state
 * the library keeps between calls; set it before the first training call, from one thread.
 * (The BatchNorms of hvpr_bn_* take the other route: their sums / apply halves are separate entry points.) */
typedef int (*hvpr_allreduce_fn)(double *buf, int n, hvpr_stream_t stream, void *ctx);
void hvpr_set_batchnorm_allreduce(hvpr_allreduce_fn fn, void *ctx);

/* ---------------------------------------------------------------------------------------------
 * a1  Voxelizer.  Replaces spconv.utils.VoxelGenerator[V2].generate as called from
 *     pcdet/datasets/processor/data_processor.py:43-75 (CPU dataloader in the reference).
 *     Bit-exact first-touch semantics: voxel id = order of first appearance in the point array,
 *     first `max_points` points of a voxel kept in point order, coords = floor((p-lo)/vs) in fp32.
 *
 *     points        [n_points, point_stride] f32; xyz at columns xyz_col..xyz_col+2; the n_feat
 *                   columns starting at xyz_col are copied into the voxels (n_feat >= 3).
 *     frame_offsets [batch+1] i32 device; frame b owns points [frame_offsets[b], frame_offsets[b+1]).
 *     cap_mode      0 = VoxelGeneratorV2 (`continue` once max_voxels is reached),
 *                   1 = VoxelGenerator v1 / tools/vis.py:47-48 (`break`).
 *     voxels        [capacity, max_points, n_feat] f32 out, zero padded.
 *     coords        [capacity, 4] i32 out  [b, z, y, x]   (dataset.py:161-166 prepends b)
 *     num_points    [capacity] i32 out
 *     voxel_offsets [batch+1] i32 out; frame b produced rows [voxel_offsets[b], voxel_offsets[b+1]).
 *     capacity      rows available in the three outputs; >= sum_b min(N_b, max_voxels) is always enough.
 *     max_points <= 63.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_voxelize_workspace_bytes(int max_batch, int max_points, int nx, int ny, int nz);
/* one-time (and after any failed call): puts the workspace in its idle state.  A workspace sized and reset for
 * (max_batch, max_points) serves every call with batch <= max_batch and n_points <= max_points on the same grid;
 * each call returns it to idle. */
int hvpr_voxelize_workspace_reset(void *workspace, size_t workspace_bytes, int max_batch, int max_points, int nx, int ny,
                                  int nz, hvpr_stream_t stream);
/* SYNCHRONISES `stream` and reads the workspace's error word (dimensions as it was sized with): HVPR_OK, or HVPR_ERR_TIMEOUT when a
 * one-launch index kernel (hvpr_encode_fwd_f32, index_mode 1) gave up a wait since the last reset — that call and every later
 * mode-1 call on this workspace reported zero pillars; reset the workspace before using it again.  Call it where the caller
 * synchronises anyway (the detector does when it reads its results back). */
int hvpr_voxelize_workspace_status(const void *workspace, size_t workspace_bytes, int max_batch, int max_points, int nx, int ny,
                                   int nz, hvpr_stream_t stream);
int hvpr_voxelize_f32(const float *points, int n_points, int point_stride, int xyz_col, int n_feat,
                      const int32_t *frame_offsets, int batch, float lo_x, float lo_y, float lo_z, float vs_x,
                      float vs_y, float vs_z, int nx, int ny, int nz, int max_points, int max_voxels, int cap_mode,
                      float *voxels, int32_t *coords, int32_t *num_points, int32_t *voxel_offsets, int capacity,
                      void *workspace, size_t workspace_bytes, int ws_max_batch, int ws_max_points,
                      hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a2  Pillar VFE, eval mode (BatchNorm folded by the caller).  Replaces
 *     PillarVFE_Scale.forward, pcdet/models/backbones_3d/vfe/pillar_vfe.py:184-221 (+ PFNLayer :29-49)
 *     for USE_ABSLOTE_XYZ=True, WITH_DISTANCE=False, NUM_FILTERS=[32,64], NUM_SCALE_FEATURES=[16,32],
 *     4 raw point features.
 *
 *     voxels [M, P, 4] f32 zero padded (P <= 32), num_points [M] i32, coords [M,4] i32 [b,z,y,x].
 *     w0 [16,10] b0 [16]: folded Linear(10->16)+BN;  w1 [64,32] b1 [64]: folded Linear(32->64)+BN;
 *     ws0 [16,5] bs0 [16], ws1 [32,16] bs1 [32]: the folded scale-stream layers.
 *     pillar_features [M,64], pillar_scale_features [M,32], pillar_mask [M,P] (may be NULL) f32 out.
 *     m_device: optional device i32 holding the live row count (<= M); NULL means M rows.
 *     A row with num_points == 0 is unspecified (the reference divides by zero) but reads and writes only its own cells; a
 *     count above P is taken as P, a negative one as 0.
 * ------------------------------------------------------------------------------------------- */
int hvpr_pillar_vfe_fwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P,
                            const int32_t *m_device, float vs_x, float vs_y, float vs_z, float off_x, float off_y,
                            float off_z, const float *w0, const float *b0, const float *w1, const float *b1,
                            const float *ws0, const float *bs0, const float *ws1, const float *bs1,
                            float *pillar_features, float *pillar_scale_features, float *pillar_mask,
                            hvpr_stream_t stream);

/* a2 (plain)  The pillar encoder of plain PointPillars, eval mode (BatchNorm folded by the caller).  Replaces PillarVFE.forward,
 *     pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-124 (+ PFNLayer :29-49), for ONE PFN layer (NUM_FILTERS=[c_out]),
 *     USE_ABSLOTE_XYZ=True, WITH_DISTANCE=False, 4 raw point features.  Arguments as in hvpr_pillar_vfe_fwd_f32:
 *     voxels [M, P, 4] f32 zero padded, num_points [M] i32, coords [M,4] i32 [b,z,y,x]; m_device: optional device i32 holding the
 *     live row count (<= M; rows at or past it are unspecified), NULL means M rows; vs_* / off_*: voxel size and
 *     (voxel_size / 2 + range minimum) per axis.  w [c_out,10] b [c_out]: the folded Linear(10->c_out)+BN.
 *     pillar_features [M,c_out], pillar_mask [M,P] (may be NULL) f32 out.
 *     Per slot p the ten features are the raw 4, xyz - mean, xyz - (cell * vs + off), all times (p < num_points[m]), with
 *     mean = (sum over ALL P slots) / float(num_points[m]); out[m,c] = max over ALL P slots of relu(w[c] . f[p] + b[c]) — a padded
 *     slot contributes relu(b[c]), as in the reference.  A row with num_points == 0 is unspecified (the reference divides by zero)
 *     but reads and writes only its own cells.
 *     c_out in {32, 64, 128} and 1 <= P <= 32, anything else HVPR_ERR_UNSUPPORTED; the arguments are checked before any device
 *     call; M == 0 returns HVPR_OK without a launch.  One launch, no host read, no allocation: capturable. */
int hvpr_pillar_vfe_plain_fwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P,
                                  const int32_t *m_device, float vs_x, float vs_y, float vs_z, float off_x, float off_y,
                                  float off_z, const float *w, const float *b, int c_out, float *pillar_features,
                                  float *pillar_mask, hvpr_stream_t stream);

/* a2 (training)  The two PFN layers of PillarVFE_Scale with BATCH-statistics BatchNorm (pillar_vfe.py:184-221, PFNLayer :29-49:
 *     linear -> BatchNorm1d over all M * P slots, padded ones included -> ReLU -> max over the slots -> concat), forward and
 *     backward, for the same fixed shapes as hvpr_pillar_vfe_fwd_f32 (P == 32).  No (M, P, C) tensor is materialised: every pass
 *     recomputes from the voxels (three forward passes, two backward passes + two for the statistics).
 *     w0 [16,10], gamma0 / beta0 [16], w1 [64,32], gamma1 / beta1 [64]: the Linear weights and BatchNorm affine parameters;
 *     eps: BatchNorm's; vs_* / off_*: voxel size and (voxel_size / 2 + range minimum) per axis as in the eval entry point.
 *     fwd: pillar_features [M,64]; mean0 / var0 [16], mean1 / var1 [64] = batch mean and BIASED variance of both layers (for the
 *          caller's running statistics).
 *     bwd: d_pillar_features [M,64] -> dw0 [16,10], dgamma0, dbeta0 [16], dw1 [64,32], dgamma1, dbeta1 [64] (overwritten; the
 *          batch statistics are recomputed, the workspace carries no state between calls).  The voxels get no gradient.
 *     Deterministic (fixed-order sums, finished in double).  workspace: hvpr_pillar_vfe_train_workspace_bytes(). */
size_t hvpr_pillar_vfe_train_workspace_bytes(void);
int hvpr_pillar_vfe_train_fwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P, const float *w0,
                                  const float *gamma0, const float *beta0, const float *w1, const float *gamma1, const float *beta1,
                                  float eps, float vs_x, float vs_y, float vs_z, float off_x, float off_y, float off_z,
                                  float *pillar_features, float *mean0, float *var0, float *mean1, float *var1, void *workspace,
                                  size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_pillar_vfe_bwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P, const float *w0,
                            const float *gamma0, const float *beta0, const float *w1, const float *gamma1, const float *beta1, float eps,
                            float vs_x, float vs_y, float vs_z, float off_x, float off_y, float off_z, const float *d_pillar_features,
                            float *dw0, float *dgamma0, float *dbeta0, float *dw1, float *dgamma1, float *dbeta1, void *workspace,
                            size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a3  Memory read-out, eval branch.  Replaces MemoryUnit_Agg.forward (eval),
 *     pcdet/models/backbones_2d/map_to_bev/memory_module.py:60-77: logits = f.W^T, top-k items,
 *     softmax over the k selected logits, weighted sum of the k items.
 *     f [M,64], bank [n_items,64] -> out [M,64]; topk_idx [M,k] i32 (may be NULL; the k selected ids, order unspecified).
 *     k <= 32, channels == 64.
 *     bank_packed (REQUIRED): the output of hvpr_memory_bank_pack_f32 for the same bank (only that function may produce it) — IEEE fp16 tiles in the matrix-core
 *     operand layout + the 64 channel maxima max_j |bank[j][c]|; pack once per weight update.  The kernel pre-filters on the
 *     fp16 matrix cores (v_mfma_f32_16x16x32_f16) with a rigorous rounding-error bound and re-checks the ~30 surviving candidates per row in exact
 *     fp32 from `bank` (logit = butterfly-tree sum of the 64 fp32 products), so the selected ids are the exact fp32 top-k
 *     (value descending, id ascending on ties); the k selected rows are read from `bank` too.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_memory_bank_packed_floats(int n_items);   /* size of the packed copy in floats: ceil(n_items/16) * 512 + 128 */
int hvpr_memory_bank_pack_f32(const float *bank, int n_items, float *packed, hvpr_stream_t stream);
int hvpr_memory_readout_fwd_f32(const float *f, int M, const int32_t *m_device, const float *bank, const float *bank_packed,
                                int n_items, int k, float *out, int32_t *topk_idx, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a4  Scatter to the dense BEV canvases.  Replaces the eval branch of
 *     PointPillarScatter_Agg_Memory_1_scale.forward, map_to_bev/pointpillar_scatter.py:169-222
 *     (and plain PointPillarScatter :5-37 when memory/scale inputs are NULL).
 *     The canvases are written channels-last: spatial [B, ny, nx, c_pillar + c_mem],
 *     spatial_scale [B, ny, nx, c_scale] — logically (B, C, ny, nx) tensors in torch's
 *     channels_last memory format.  Every element is written exactly once (zeros included).
 *     coords [M,4] i32 [b,z,y,x]; cell_map: workspace of B*ny*nx i32.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_scatter_workspace_bytes(int batch, int nx, int ny);
int hvpr_scatter_bev_fwd_f32(const float *pillar_features, int c_pillar, const float *memory_features, int c_mem,
                             const float *scale_features, int c_scale, const int32_t *coords, int M,
                             const int32_t *m_device, int batch, int nx, int ny, float *spatial,
                             float *spatial_scale, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* a3+a4 fused, the form PointPillarScatter_Agg_Memory_1_scale.forward (eval, pointpillar_scatter.py:169-222) uses: the
 *     memory read-out also fills the scatter cell map (one launch less than the two calls above, same results).
 *     Fixed channel counts 64 (pillar) + 64 (memory) + 32 (scale).  memory_features [M,64] is an output. */
int hvpr_memory_scatter_fwd_f32(const float *pillar_features, const float *scale_features, const int32_t *coords, int M,
                                const int32_t *m_device, const float *bank, const float *bank_packed, int n_items, int k, int batch,
                                int nx, int ny,
                                float *memory_features, float *spatial, float *spatial_scale, void *workspace,
                                size_t workspace_bytes, hvpr_stream_t stream);

/* a1..a4 fused — points to BEV canvases in five launches (three with index_mode 1), the form the detector's eval forward uses when it is handed raw
 *     points.  Same results, bit for bit, as hvpr_voxelize_f32 -> hvpr_pillar_vfe_fwd_f32 -> hvpr_memory_scatter_fwd_f32
 *     (data_processor.py:43-75, pillar_vfe.py:184-221, memory_module.py:60-77, pointpillar_scatter.py:169-222) with
 *       - the voxel gather fused into the VFE (the padded `voxels` tensor becomes an optional OUTPUT, may be NULL),
 *       - the pillar / scale / memory cells of the canvases written by the VFE and the read-out themselves, and every other
 *         cell cleared by extra workgroups of the (latency-bound) VFE launch: no scatter pass, no cell map.
 *     Arguments as in the three separate calls; n_feat must be 4, nz 1, max_points <= 32, channels 64 + 64 + 32.
 *     voxel_offsets[batch] is the live pillar count M (device word); rows >= M of the per-pillar outputs are unspecified.
 *     capacity below M truncates: the first `capacity` rows are written, the canvas cells of the dropped pillars stay zero.
 *     index_mode selects the launch form of the index phase (cell keys -> voxel ranks -> arena), same results either way:
 *       0  three launches (K1 keys, K2 rank scan, K3 arena fill).  No workgroup waits for another one beyond the scan's look-back:
 *          safe for any number of calls in flight on any number of streams, and for several processes sharing a GPU.  The default
 *          every C caller should use unless it has read the next paragraph.
 *       1  ONE launch (up to 32 768 points; beyond that mode 0 is taken) whose at most 32 owner workgroups meet at two grid
 *          barriers on the compute units of one XCD — 2.6 us less per hvpr_car frame.  Owners that are resident wait for the ones
 *          that are not, so two such launches in flight at once could each hold compute units the other one needs.  The library
 *          rules that out inside a process: it takes the one-launch form only if the previous one-launch kernel on this device
 *          went to the same stream or has completed (one event query), and falls back to the three launches otherwise.  It
 *          cannot see other processes, and it cannot decide anything inside a stream capture (a captured call with index_mode 1
 *          always holds the one-launch form: replay such graphs one at a time per device — the detector's frame pipeline has one
 *          encode lane).  Every wait inside the kernel is bounded (2 s): a launch that could not complete raises a sticky error word
 *          in the workspace, reports zero pillars (voxel_offsets all 0; every other output of that call is unspecified), leaves the
 *          barrier words idle, and so does every later mode-1 call on that workspace until hvpr_voxelize_workspace_reset;
 *          hvpr_voxelize_workspace_status reads the word — check it wherever results are read back.
 *     pillar_mask may be NULL.  workspace: hvpr_voxelize_workspace_bytes / _reset, as for hvpr_voxelize_f32.
 *     Weight / bias pointers 16-byte aligned.
 *     canvas_state (may be NULL): [batch * ny * nx] bytes that travel with ONE pair of canvases the caller keeps between calls.
 *     NULL: every element of both canvases is written (zeros included), the canvases may hold anything on entry.
 *     Non-NULL: 1 = the cell holds a pillar of the previous call, and the caller guarantees the canvases are zero wherever it
 *     says 0 (start: canvases and state all zero).  Only the stale cells are then cleared (~2.4 MB instead of 47 MB per
 *     hvpr_car frame) and the state is updated; results are the same dense canvases. */
int hvpr_encode_fwd_f32(const float *points, int n_points, int point_stride, int xyz_col, int n_feat,
                        const int32_t *frame_offsets, int batch, float lo_x, float lo_y, float lo_z, float vs_x, float vs_y,
                        float vs_z, int nx, int ny, int nz, int max_points, int max_voxels, int cap_mode, float off_x,
                        float off_y, float off_z, const float *w0, const float *b0, const float *w1, const float *b1,
                        const float *ws0, const float *bs0, const float *ws1, const float *bs1, const float *bank,
                        const float *bank_packed, int n_items, int k, float *voxels, int32_t *coords, int32_t *num_points, int32_t *voxel_offsets,
                        int capacity, float *pillar_features, float *pillar_scale_features, float *pillar_mask,
                        float *memory_features, float *spatial, float *spatial_scale, uint8_t *canvas_state, void *workspace,
                        size_t workspace_bytes, int ws_max_batch, int ws_max_points, int index_mode, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a5/a6  BEV backbone + head convolutions: implicit GEMM on the fp32 matrix cores, NHWC.
 *     Replaces the cuDNN convolutions behind BaseBEVBackbone_Scale.forward (eval),
 *     pcdet/models/backbones_2d/base_bev_backbone.py:280-315 — ZeroPad2d(1)+Conv3x3(s)+BN+ReLU (:154-169),
 *     the shared SFM step x_att = gate*ReLU(BN(conv(x_att))) + x_att (:291-295), ConvTranspose2d(k=s)+BN+ReLU
 *     (:177-188) written into its slice of the concat (:303-304) — and the three 1x1 head convolutions of
 *     AnchorHeadSingle.forward, pcdet/models/dense_heads/anchor_head_single.py:112-121.
 *
 *     in        [N, H, W, Cin] f32 (Cin % 8 == 0)
 *     w_packed  [taps, Cin/8, 2, cout_pad, 4] f32 (input channel = 8*chunk + 4*half + i), BatchNorm scale folded in;
 *               taps = 9 (3x3, pad 1) or 1 (1x1).
 *               For up > 1 (ConvTranspose2d with kernel == stride == up) taps = 1 and the gemm column is
 *               (ky*up + kx)*cout + co.
 *     bias      [cout_pad] f32 by gemm column (folded BatchNorm shift or the conv bias)
 *     gate/resid  both NULL, or gate [N, OH, OW] and resid [N, OH, OW, resid_cstride]: y = gate*y + resid
 *     out       [N, OH*up, OW*up, out_cstride] f32, channels written at out_coff .. out_coff+cout
 *     tile_cfg  0: 128 px x 128 ch   1: 64 px x 64 ch   2: 128 px x 64 ch   (cout_pad % tile channels == 0)
 * ------------------------------------------------------------------------------------------- */
int hvpr_conv2d_nhwc_f32(const float *in, int N, int H, int W, int Cin, const float *w_packed, const float *bias,
                         int taps, int stride, int cout, int cout_pad, int up, int relu, const float *gate,
                         const float *resid, int resid_cstride, float *out, int out_cstride, int out_coff,
                         int tile_cfg, hvpr_stream_t stream);
/* Walk table (optional).  A workgroup of the persistent kernel otherwise derives every item (image, pixel tile, channel tile) of its
 * walk by integer divisions; a table holds them, one 8-byte entry per walk step, built once per (N, H, W, taps, stride, cout_pad,
 * tile_cfg) into caller-owned device memory of hvpr_conv2d_tab_bytes bytes (0: no table for these arguments) by
 * hvpr_conv2d_tab_build.  hvpr_conv2d_nhwc_tab_f32 is hvpr_conv2d_nhwc_f32 with `table` = the table of exactly this shape, or NULL
 * for the in-kernel decode; the result is bit-identical either way.  The table must stay valid until the launch has run. */
size_t hvpr_conv2d_tab_bytes(int N, int H, int W, int taps, int stride, int cout_pad, int tile_cfg);
int hvpr_conv2d_tab_build(int N, int H, int W, int taps, int stride, int cout_pad, int tile_cfg, void *table, hvpr_stream_t stream);
int hvpr_conv2d_nhwc_tab_f32(const float *in, int N, int H, int W, int Cin, const float *w_packed, const float *bias,
                             int taps, int stride, int cout, int cout_pad, int up, int relu, const float *gate,
                             const float *resid, int resid_cstride, float *out, int out_cstride, int out_coff,
                             int tile_cfg, const void *table, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a5  SpatialAttention gate.  Replaces ChannelPool + ConvLayer(2->1, 3x3, bias) + BatchNorm + sigmoid of
 *     pcdet/models/backbones_2d/spatial_attention.py:47-62.  y [N,H,W,C] NHWC -> gate [N,H,W].
 *     w18: conv weight (1,2,3,3) flattened [max-channel 9 taps | mean-channel 9 taps]; bn_scale/bn_shift: folded BN.
 * ------------------------------------------------------------------------------------------- */
int hvpr_spatial_gate_f32(const float *y, int N, int H, int W, int C, const float *w18, float conv_bias, float bn_scale,
                          float bn_shift, float *gate, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a7  Anchors + box decode + direction fix + class sigmoid/max.  Replaces
 *     AnchorHeadTemplate.generate_predicted_boxes (dense_heads/anchor_head_template.py:293-340),
 *     ResidualCoder.decode_torch (utils/box_coder_utils.py:45-77), limit_period (utils/common_utils.py:20-23) and the
 *     sigmoid + max over classes of Detector3DTemplate.post_processing (detectors/detector3d_template.py:206-207,241-246).
 *     head [N,H,W, n_anchor*(n_class + 7 + n_dir_bins)] = [cls | box | dir] NHWC (output of the three 1x1 convs);
 *     x_shifts [W], y_shifts [H]: anchor centres exactly as AnchorGenerator's arange (anchor_generator.py:34-39);
 *     anchor_table [n_anchor,5] = z centre, dx, dy, dz, rotation.  Anchor id = (y*W + x)*n_anchor + a.
 *     Outputs: batch_cls_preds [N,A,n_class] (may be NULL), batch_box_preds [N,A,7], scores [N,A] (may be NULL),
 *     labels [N,A] i32, 1-based (may be NULL).
 * ------------------------------------------------------------------------------------------- */
int hvpr_head_decode_f32(const float *head, int N, int H, int W, int head_channels, int n_anchor, int n_class,
                         int n_dir_bins, const float *x_shifts, const float *y_shifts, const float *anchor_table,
                         float dir_offset, float dir_limit_offset, float period, float *batch_cls_preds,
                         float *batch_box_preds, float *scores, int32_t *labels, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a8  Score filter + top-k.  Replaces `scores >= thresh`, torch.topk and mask.nonzero() of
 *     class_agnostic_nms, pcdet/models/model_utils/model_nms_utils.py:8-16,22-24.
 *     scores [batch, n_scores]; order [batch, pre_max] i32 = ids sorted by (score desc, id asc);
 *     sorted_scores [batch, pre_max] (may be NULL); counts [batch] i32 = min(#passing, pre_max).
 *     use_thresh = 0 keeps every non-NaN score.  pre_max <= 8192.  -0.0 and +0.0 are equal scores (ties go by id);
 *     sorted_scores holds +0.0 for both.
 *     workspace: zero-filled by the caller ONCE; every call returns its counters, histogram and rank array to zero (no
 *     per-call memset).  Calls that share a workspace pass the same batch; n_scores may change from call to call.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_score_topk_workspace_bytes(int batch, int n_scores);
int hvpr_score_topk_f32(const float *scores, int batch, int n_scores, float score_thresh, int use_thresh, int pre_max,
                        int32_t *order, float *sorted_scores, int32_t *counts, void *workspace, size_t workspace_bytes,
                        hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a8  Rotated-BEV NMS and pairwise overlaps.  Replaces the absent pcdet/ops/iou3d_nms natives (setup.py:53-62):
 *     nms_gpu (call site model_nms_utils.py:17-19), boxes_overlap_bev_gpu / boxes_iou_bev / boxes_iou3d_gpu
 *     (detectors/detector3d_template.py:298,303).  Boxes [x,y,z,dx,dy,dz,heading], rows `box_stride` floats apart.
 *     hvpr_nms_bev_f32: candidate i is boxes[order ? order[i] : i], candidates already in descending score;
 *       n_device (may be NULL) holds the live count <= n_max (<= 16384); IoU > thresh suppresses (strict);
 *       keep[0..keep_count) = kept candidate positions, or order[position] when map_through_order != 0;
 *       at most max_keep are produced (NMS_POST_MAXSIZE).  A workspace of hvpr_nms_workspace_bytes(n) bytes serves every
 *       n_max <= n.
 *     hvpr_boxes_pairwise_f32: mode 0 BEV overlap area, 1 BEV IoU, 2 3D IoU; out [n, m]; rows 7 floats apart.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_nms_workspace_bytes(int n_max);
int hvpr_nms_bev_f32(const float *boxes, int box_stride, const int32_t *order, const int32_t *n_device, int n_max,
                     float thresh, int max_keep, int map_through_order, int32_t *keep, int32_t *keep_count,
                     void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
/* tail of post_processing (detector3d_template.py:255-259): out_*[r] = *[keep[r]] for r < max_keep (boxes 7 columns; labels and
 * the selected ids widened to int64 as the reference returns them); keep[] rows past the live count must hold valid ids */
int hvpr_gather_predictions_f32(const float *boxes, int box_stride, const float *scores, const int32_t *labels,
                                const int32_t *keep, int max_keep, float *out_boxes, float *out_scores, int64_t *out_labels,
                                int64_t *out_selected, hvpr_stream_t stream);
int hvpr_boxes_pairwise_f32(const float *boxes_a, int n, const float *boxes_b, int m, int mode, float *out,
                            hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a8  Batched rotated NMS: S independent candidate lists (the frames of a batch, or every (frame, class) of the
 *     MULTI_CLASSES_NMS branch) in ONE call, five launches whatever S is.  The single forms above are this with one segment.
 *     Segment s reads the box table at boxes + (s / segments_per_table) * table_stride floats; its candidate i is row
 *     order ? order[s * n_max + i] : i of that table; n_device[s] candidates are live (clamped to n_max; NULL: all n_max).
 *     segments_per_table = 1: one table per segment (a batch of frames); = num_class: the classes of a frame rank one table.
 *     keep [S, max_keep], keep_count [S]: per segment exactly what hvpr_nms_bev_f32 gives for that segment alone.
 *     n_segments == 0: nothing is done; n_max == 0: the S counts are zeroed.  n_max <= 16384, n_segments <= 65535.
 *     Workspace: S private copies of the single form's layout, 256-byte aligned each (about 19.5 MB per segment at
 *     n_max = 4096); hvpr_nms_bev_batched_workspace_bytes(1, n) == hvpr_nms_workspace_bytes(n), and a workspace sized for
 *     (S, n) serves every call with at most S segments and n_max <= n.
 *     hvpr_gather_predictions_batched_f32: out_*[s, r] = *[keep[s, r]] for r < max_keep; boxes are addressed like the NMS's
 *     (table_stride, segments_per_table); scores and labels are one row per segment, score_stride elements apart.
 *     hvpr_gather_predictions_multiclass_f32: the records of the MULTI_CLASSES_NMS branch without a host read.  keep
 *     [n_frames * n_class, max_keep] and keep_count [n_frames * n_class] are the batched NMS's over the class-major score rows
 *     [n_frames * n_class, score_stride] (row b * n_class + k: class k of frame b, ranking box table b).  Frame b's rows are the
 *     kept candidates of class 0, then class 1, ..., each in keep order; class k starts at the sum of min(keep_count, max_keep)
 *     over the classes in front of it (computed in the kernel); label = k + 1, score = class k's of the anchor.  out_boxes
 *     [n_frames, n_class * max_keep, 7], out_scores / out_labels / out_selected [n_frames, n_class * max_keep], out_count
 *     [n_frames] = the frame's total; every row past it holds anchor 0 of class 0 (label 1, selected 0).  One launch;
 *     n_frames == 0: nothing is done; n_class == 0 or max_keep == 0: the counts are zeroed.  n_frames <= 65535.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_nms_bev_batched_workspace_bytes(int n_segments, int n_max);
int hvpr_nms_bev_batched_f32(const float *boxes, int box_stride, long long table_stride, int segments_per_table,
                             const int32_t *order, const int32_t *n_device, int n_segments, int n_max, float thresh,
                             int max_keep, int map_through_order, int32_t *keep, int32_t *keep_count, void *workspace,
                             size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_gather_predictions_batched_f32(const float *boxes, int box_stride, long long table_stride, int segments_per_table,
                                        const float *scores, const int32_t *labels, long long score_stride,
                                        const int32_t *keep, int n_segments, int max_keep, float *out_boxes,
                                        float *out_scores, int64_t *out_labels, int64_t *out_selected, hvpr_stream_t stream);
int hvpr_gather_predictions_multiclass_f32(const float *boxes, int box_stride, long long table_stride, const float *scores,
                                           long long score_stride, const int32_t *keep, const int32_t *keep_count, int n_frames,
                                           int n_class, int max_keep, float *out_boxes, float *out_scores, int64_t *out_labels,
                                           int64_t *out_selected, int32_t *out_count, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3  KITTI AP on the device (hvpr_amd/kitti_eval_device.py; the host evaluator hvpr_amd/kitti_eval.py is the yardstick).
 *     All F frames of a split lie end to end: frame f owns rows off[f] .. off[f + 1) of its table and the nd_f x ng_f pairs
 *     pair_off[f] .. pair_off[f + 1), pair p = (detection i, ground truth j) = divmod(p - pair_off[f], ng_f).  The offset
 *     arrays are DEVICE int64 [F + 1] and must be consistent (pair_off[F] == n_pairs); they are not checked on the device.
 *     hvpr_boxes_pairwise_ragged_f32: mode 0 of hvpr_boxes_pairwise_f32 for every frame in one launch, bit for bit: out[p] =
 *       overlap area of row a_off[f] + i of boxes_a and row b_off[f] + j of boxes_b (7 floats per row).
 *     hvpr_kitti_overlaps_f64: out[p] = frame_overlap of the host in double.  Annotation rows are 16 doubles: bbox[4], alpha,
 *       location[3], dimensions[3], rotation_y, occluded, truncated, score, pad.  metric 0 bbox IoU (inter may be NULL), 1 BEV,
 *       2 3-D: `inter` is the ragged fp32 intersection of the (x, z, l, w, -rotation_y) rectangles.
 *     hvpr_kitti_match_f64: greedy matching of every (frame, class m, difficulty l, overlap set k), combo = (m * 3 + l) * n_sets
 *       + k.  classes [n_classes <= 8] (ids 0..5 of Car, Pedestrian, Cyclist, Van, Person_sitting, Truck) and min_overlaps
 *       [n_sets <= 4][n_classes] (>= 0) are HOST arrays; gt_cls / dt_cls hold those ids (or -1), gt_dontcare one byte per box.
 *       At most 4096 detections per frame (checked by the caller).
 *       pass 0 (thresholds): tp_score [combos][n_gt_total] = score of the detection matched to each ground truth as a true
 *         positive, else NaN; n_valid [n_classes][3] = ground truths to evaluate.  thresholds .. workspace are unused.
 *       pass 1 (counts): thresholds [combos][n_thresh] with thresh_count [combos] live entries each (device); counts [combos]
 *         [n_thresh][3] = tp, fp, fn summed over the frames, sim [combos][n_thresh] = the orientation similarity of the true
 *         positives (zeros, and sim may be NULL, when compute_aos == 0), zeros past thresh_count.  Integer sums, and the similarity is summed in one fixed order:
 *         two runs give the same bits.  workspace: hvpr_kitti_match_workspace_bytes(...) bytes.
 * ------------------------------------------------------------------------------------------- */
int hvpr_boxes_pairwise_ragged_f32(const float *boxes_a, const float *boxes_b, const int64_t *a_off, const int64_t *b_off,
                                   const int64_t *pair_off, int n_frames, long long n_pairs, float *out, hvpr_stream_t stream);
int hvpr_kitti_overlaps_f64(const double *gt_rows, const double *dt_rows, const float *inter, const int64_t *gt_off,
                            const int64_t *dt_off, const int64_t *pair_off, int n_frames, long long n_pairs, int metric,
                            double *out, hvpr_stream_t stream);
size_t hvpr_kitti_match_workspace_bytes(int n_frames, int n_classes, int n_sets, int n_thresh);
int hvpr_kitti_match_f64(const double *gt_rows, const int32_t *gt_cls, const uint8_t *gt_dontcare, const double *dt_rows,
                         const int32_t *dt_cls, const int64_t *gt_off, const int64_t *dt_off, const int64_t *pair_off,
                         int n_frames, long long n_gt_total, const double *overlaps, int metric, int pass,
                         const int32_t *classes, int n_classes, const double *min_overlaps, int n_sets,
                         const double *thresholds, const int32_t *thresh_count, int n_thresh, int compute_aos,
                         double *tp_score, int32_t *n_valid, int32_t *counts, double *sim, void *workspace,
                         size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f5  Evaluation epilogue on the device (hvpr_amd/eval_loop.py): from the padded records of post_processing(sync=False) to recall
 *     counters and KITTI annotation rows, a batch of B frames per call.  Neither entry point synchronises or reads the device;
 *     every check is made on the host and a refused call launches nothing.
 *     hvpr_recall_record_f32: generate_recall_record (detector3d_template.py:276-318) for every frame.  pred_boxes [B, P, 7] with
 *       pred_count[b] live rows (device, clamped to 0..P); gt_boxes [B, G, C >= 7] padded with zero rows; thresholds [T <= 8] is a
 *       HOST array (more: HVPR_ERR_UNSUPPORTED).  counts [B, 1 + T] i32: the frame's ground-truth count, then per threshold the
 *       ground truths whose best 3-D IoU (mode 2 of hvpr_boxes_pairwise_f32, bit for bit) over the live predictions is > t.
 *       Ground-truth count: trailing rows whose left-to-right fp32 sum of the C columns is 0 are cut, row 0 never is (a table of
 *       zero rows counts one box, as in the reference); G == 0 counts nothing.  A frame without live predictions recalls nothing.
 *       best_iou [B, G] (may be NULL): that best IoU; 0 for cut rows and for frames without predictions.
 *     hvpr_prediction_annos_f32: generate_prediction_dicts (kitti_dataset.py:246-320, box_utils.py:152-235) for every frame, in
 *       fp32, widened at the store.  pred_boxes [B, P, 7], pred_scores [B, P], pred_labels [B, P] i64 (1-based), pred_count [B];
 *       calib [B, 26] f32 on the device: the 4 x 3 product V2C^T R0^T row-major, P2 3 x 4 row-major, image height, image width;
 *       class_of_label [n_labels <= 16] a HOST map from label - 1 to the evaluator's class id (other labels give -1).  Frame b's
 *       live rows go to rows row_base[0] + (live rows of frames before b) .. of the caller's tables: dt_rows [cap, 16] f64 (the
 *       annotation row of f3), dt_cls / dt_label [cap] i32, dt_box7 [cap, 7] f32 (x, z, 0, l, w, 1, -rotation_y), boxes_lidar
 *       [cap, 7] f32 (z is the bottom centre's: the reference lowers it in the array it returns); dt_off[frame_base + b + 1] = the
 *       row after frame b's (dt_off holds max_frames + 1 int64 words, dt_off[0] is the caller's).  row_base is a DEVICE word, advanced by a
 *       second launch after the first.  Rows at or past cap are not written; *overflow is then set to 1 and offsets stop at cap.
 * ------------------------------------------------------------------------------------------- */
int hvpr_recall_record_f32(const float *pred_boxes, const int32_t *pred_count, int B, int P, const float *gt_boxes, int G, int C,
                           const float *thresholds, int T, int32_t *counts, float *best_iou, hvpr_stream_t stream);
int hvpr_prediction_annos_f32(const float *pred_boxes, const float *pred_scores, const int64_t *pred_labels,
                              const int32_t *pred_count, int B, int P, const float *calib, const int32_t *class_of_label,
                              int n_labels, int64_t *row_base, long long cap, int frame_base, int max_frames, double *dt_rows,
                              int32_t *dt_cls, int32_t *dt_label, float *dt_box7, float *boxes_lidar, int64_t *dt_off,
                              int32_t *overflow, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a9 (training)  PointNet++ index ops.  Replace the absent natives of pcdet/ops/pointnet2/pointnet2_batch (setup.py:94-109)
 *     behind PointnetSAModuleMSG / PointnetFPModule (pcdet/models/backbones_3d/pointnet2_backbone.py:27-34,43-47,82,86-89).
 *     Indices only (no gradient); tie rule: lowest index.  Distances are fp32 (dx*dx + dy*dy) + dz*dz.
 *     hvpr_furthest_point_sample_f32: xyz [B,N,3] -> idx [B,npoint] i32, first pick = index 0, N <= 32768.
 *     hvpr_ball_query_f32: first nsample points (index order) with d2 < radius^2; the first hit pre-fills all slots; zeros
 *                          when there is none.  xyz [B,N,3], new_xyz [B,M,3] -> idx [B,M,nsample] i32.
 *     hvpr_three_nn_f32:   unknown [B,n,3], known [B,m,3] -> dist [B,n,3] (sqrt of d2, ascending), idx [B,n,3] i32.
 * ------------------------------------------------------------------------------------------- */
int hvpr_furthest_point_sample_f32(const float *xyz, int B, int N, int npoint, int32_t *idx, hvpr_stream_t stream);
int hvpr_ball_query_f32(const float *xyz, const float *new_xyz, int B, int N, int M, float radius, int nsample, int32_t *idx,
                        hvpr_stream_t stream);
int hvpr_three_nn_f32(const float *unknown, const float *known, int B, int n, int m, float *dist, int32_t *idx,
                      hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a9 (training)  Differentiable gathers of the point stream, in the reference's channel-major layout.  Replace
 *     grouping_operation / gather_operation / three_interpolate of the absent
 *     pcdet/ops/pointnet2/pointnet2_batch natives (setup.py:94-109; used by PointnetSAModuleMSG / PointnetFPModule,
 *     pcdet/models/backbones_3d/pointnet2_backbone.py:27-34,43-47,82,86-89).
 *     hvpr_group_points_f32:        features [B,C,N], idx [B,npoint,nsample] i32 -> out [B,C,npoint,nsample]
 *                                   (nsample == 1: gather_operation).
 *     hvpr_three_interpolate_f32:   features [B,C,m], idx / weight [B,n,3] -> out [B,C,n] = (f0 w0 + f1 w1) + f2 w2.
 *     Their backward is hvpr_segment_sum_rows_f32 over the transposed gradient (rows [B*npoint*nsample, C] / [B*n, C]).
 * ------------------------------------------------------------------------------------------- */
int hvpr_group_points_f32(const float *features, const int32_t *idx, int B, int C, int N, int npoint, int nsample, float *out,
                          hvpr_stream_t stream);
int hvpr_three_interpolate_f32(const float *features, const int32_t *idx, const float *weight, int B, int C, int m, int n,
                               float *out, hvpr_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * a9 (training)  Row-layout data movement around the shared MLPs of the point stream (PointnetSAModuleMSG,
 *     pcdet/models/backbones_3d/pointnet2_backbone.py:27-34; PointnetFPModule :40-47,86-89).  The MLPs themselves (1x1 convolution
 *     + train-mode BatchNorm + ReLU per layer) run on hvpr_conv2d_nhwc_f32 / hvpr_conv2d_wgrad_nhwc_f32 / hvpr_bn_* over rows
 *     [samples, cpad]: channels contiguous, zero columns up to cpad (a multiple of 8).
 *     hvpr_group_rows_f32:       QueryAndGroup(use_xyz): xyz [B,N,3], features [B,N,C] (null when C == 0), new_xyz [B,npoint,3],
 *                                idx [B,npoint,nsample] i32 -> out [B*npoint*nsample, cpad], row = [xyz[idx] - new_xyz | features[idx] | 0].
 *     hvpr_max_samples_f32:      y [G, nsample, C] -> out [G, C] = max over the samples of a group, argmax [G, C] u8 (lowest sample
 *                                on ties); nsample <= 255.        hvpr_max_samples_grad_f32: grad_out [G,C] -> grad_y [G,nsample,C].
 *     hvpr_fp_rows_f32:          PointnetFPModule's input: known [B,m,C1], idx / weight [B,n,3], skip [B,n,C2] (null when C2 == 0)
 *                                -> out [B*n, cpad], row = [(k0 w0 + k1 w1) + k2 w2 | skip | 0].
 * ------------------------------------------------------------------------------------------- */
int hvpr_group_rows_f32(const float *xyz, const float *features, const float *new_xyz, const int32_t *idx, int B, int N, int C,
                        int npoint, int nsample, int cpad, float *out, hvpr_stream_t stream);
int hvpr_max_samples_f32(const float *y, long long G, int nsample, int C, float *out, uint8_t *argmax, hvpr_stream_t stream);
int hvpr_max_samples_grad_f32(const float *grad_out, const uint8_t *argmax, long long G, int nsample, int C, float *grad_y,
                              hvpr_stream_t stream);
int hvpr_fp_rows_f32(const float *known, const int32_t *idx, const float *weight, const float *skip, int B, int m, int n, int C1,
                     int C2, int cpad, float *out, hvpr_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * a11 (training)  SpatialAttention with BATCH statistics (pcdet/models/backbones_2d/spatial_attention.py:47-63): ChannelPool ->
 *     conv3x3 2 -> 1 (+ bias) -> BatchNorm2d(1) -> sigmoid, forward and backward on NHWC y [N,H,W,C] (C % 4 == 0).  Parameters are
 *     DEVICE pointers (w18 = conv weight [1,2,3,3] flattened, conv_bias / gamma / beta one float each).
 *     fwd: pooled [N,H,W,2] (max, mean), argmax [N,H,W] i32, a [N,H,W] (conv output), stats [3] = batch mean, biased variance,
 *          1/sqrt(var + eps) of a, gate [N,H,W].     bwd: dgate [N,H,W] -> dy [N,H,W,C] (overwritten), dw18 [18], dbias, dgamma,
 *          dbeta [1] each; the batch statistics are differentiated through.  Sums: per-workgroup fp32 partials, final sums in
 *          double in a fixed order (deterministic).
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_spatial_gate_train_workspace_bytes(int N, int H, int W);
int hvpr_spatial_gate_train_fwd_f32(const float *y, int N, int H, int W, int C, const float *w18, const float *conv_bias,
                                    const float *gamma, const float *beta, float eps, float *pooled, int32_t *argmax, float *a,
                                    float *stats, float *gate, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_spatial_gate_train_bwd_f32(const float *dgate, const float *gate, const float *a, const float *stats, const float *pooled,
                                    const int32_t *argmax, const float *w18, const float *gamma, int N, int H, int W, int C,
                                    float *dy, float *dw18, float *dbias, float *dgamma, float *dbeta, void *workspace,
                                    size_t workspace_bytes, hvpr_stream_t stream);
/* a10 (training)  the index half of get_score (pointpillar_scatter.py:70-75): for every pillar row of `pillars` [M,64] the k
 * rows of `points` [N,64] with the largest dot product, idx [M,k] i32 in DESCENDING order (ties: lower index first).  N is
 * unlimited (items are walked in blocks of 2048); points_packed = hvpr_memory_bank_pack_f32(points, N) (fp16 operand tiles +
 * channel maxima).  Exact fp32 top-k through the same pre-filter + re-check scheme as hvpr_memory_readout_fwd_f32. */
int hvpr_point_pillar_topk_f32(const float *pillars, int M, const float *points, const float *points_packed, int N, int k,
                               int32_t *idx, hvpr_stream_t stream);

/* a9 / a10 (training)  Every scattering gradient, WITHOUT atomics (a point belongs to many groups — backward of QueryAndGroup /
 * grouping_operation, pointnet2_backbone.py:27-34; a known point feeds many unknown ones — backward of three_interpolate, :40-47;
 * backward of the row gather `points[idx]` (forward: hvpr_gather_rows_f32) and of the attend below, pointpillar_scatter.py:76-81):
 * dst[d][c] = sum, over the edges e = rowptr[d] .. rowptr[d+1]-1 of destination d
 * and IN THAT ORDER, of edge_w[e] * src[edge_row[e] * src_stride + src_off + c], c < C (edge_w may be null: weights 1; edge_row
 * may be null: edge e reads row e).  One
 * sequential fp32 sum per output element: two runs give the same bits.  The caller sorts the edges by destination (stable) once
 * (the Python layer's kernels.EdgePlan holds that plan and calls this twice: per chunk of 32 edges, then per destination over its
 * chunks); dst [n_dst, dst_stride] is overwritten. */
int hvpr_segment_sum_rows_f32(const float *src, long long src_stride, int src_off, int C, const int32_t *edge_row,
                              const float *edge_w, const int32_t *rowptr, long long n_dst, float *dst, long long dst_stride,
                              hvpr_stream_t stream);

/* a10 (training)  "Attend over k rows": the second half of get_score (pointpillar_scatter.py:76-81) and the aggregation of the
 * memory's training branch (memory_module.py:53-57) in one launch, without the gathered (M, k, C) tensor:
 *     w[m][j] = softmax_j( <q[m], rows[r(m,j)]> ), j < k (row maximum subtracted);   out[m] = sum_j w[m][j] * rows[r(m,j)], ascending j
 * q [M,C], rows [N,C], out [M,C], w [M,k] (what the backward needs: the weights are constants for autograd, so d rows is
 * hvpr_segment_sum_rows_f32 with src = d out, edge_row = pick / k, edge_w = w — kernels.EdgePlan.sum_rows(d out, per=k, weights=w) —
 * and there is no d q).  r(m,j) = idx[m*k+j] (i32), or
 * with idx == NULL the dense form r(m,j) = m*k+j over the caller's (M,k,C) tensor (then N must be M*k).  An index outside [0, N)
 * reads as a row of zeros.  One fixed order per output element: two runs, and the dense and the indexed form on equal row values,
 * give the same bits.  C == 64 and 1 <= k <= 32, else HVPR_ERR_UNSUPPORTED; M == 0 is a no-op; every argument check is made on the
 * host before any device call.  Row offsets are 64-bit. */
int hvpr_attend_rows_fwd_f32(const float *q, int M, const float *rows, long long N, const int32_t *idx, int k, int C, float *out,
                             float *w, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a10 (training)  MemAE memory addressing with hard shrinkage, MemoryUnit_Agg.forward training branch,
 *     map_to_bev/memory_module.py:31-48 (+ hard_shrink_relu :85-87), without materialising the (R, n_items) attention:
 *         a = softmax(x W^T), s = relu(a - l) a / (|a - l| + 1e-12), t = s / max(||s||_1, 1e-12), y = t W
 *     x [R,64] (the k positive point features of every pillar, flattened), bank [n_items <= 2048, 64], shrink_thres l > 0.
 *     fwd: y [R,64]; row_stats [R,4] (softmax max, partition sum, ||s||_1) is what the backward needs.
 *     bwd: dx [R,64] and dbank [n_items,64] (overwritten) from dy [R,64]; row_scratch [2 R] floats; no atomics — every sum
 *          is formed in a fixed order (deterministic).
 *     workspace: hvpr_memory_train_workspace_bytes(n_items), no state between calls.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_memory_train_workspace_bytes(int n_items);
int hvpr_memory_train_fwd_f32(const float *x, long long R, const float *bank, int n_items, float shrink_thres, float *y, float *row_stats,
                              void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_memory_train_bwd_f32(const float *x, const float *dy, long long R, const float *bank, int n_items, float shrink_thres,
                              const float *row_stats, float *dx, float *dbank, float *row_scratch, void *workspace,
                              size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a11 (training)  Two-stream BEV backbone, pcdet/models/backbones_2d/base_bev_backbone.py:228-279.
 *     Forward convolution and data gradient: hvpr_conv2d_nhwc_f32 (the data gradient of a stride-1 3x3 conv is the same conv
 *     on the flipped, transposed weights; stride 2 on the zero-upsampled gradient; ConvTranspose k = s as the 1x1 GEMM).
 *     hvpr_conv2d_wgrad_nhwc_f32: weight gradient on the fp32 matrix cores.  x [N,H,W,Cin] and dz [N,OH,OW,Cout] NHWC
 *         (OH = (H + 2 - 3) / stride + 1 for taps == 9 (3x3, pad 1), = H for taps == 1) -> dw [Cout, Cin, k, k] (torch layout),
 *         overwritten.  Split-K over pixel tiles into `workspace` partials, summed in a fixed order: deterministic.
 *     hvpr_conv2d_wino_wgrad_nhwc_f32: the same weight gradient for 3x3 / stride 1 / pad 1 in the Winograd F(2x2,3x3) domain
 *         (dU = sum_blocks (A dY At) . (Bt d B), dw = Gt dU G): 16 instead of 36 fp32 multiplies per 2x2 block and (co, ci) pair;
 *         x [N,H,W,Cin], dz [N,H,W,Cout] -> dw [Cout,Cin,3,3], deterministic split-K like the direct form.
 *     hvpr_conv2d_s2_dgrad_nhwc_f32: data gradient of a 3x3 stride-2 (pad 1) convolution, gathered per output-pixel parity class
 *         (1 / 2 / 2 / 4 taps) instead of a stride-1 convolution over a zero-upsampled gradient: dz [N, H, W, Cin] (the layer's
 *         output gradient; Cin = its output channels) -> dx [N, OH, OW, out_cstride] channels [out_coff, out_coff + cout) (its
 *         input's gradient; H == (OH + 2 - 3) / 2 + 1, W likewise).  w_packed = hvpr_conv2d_nhwc_f32's weight image of the layer's
 *         filter with the channel axes swapped ((cout, Cin, 3, 3), taps NOT flipped), bias [cout_pad] (zeros for a plain gradient),
 *         cout_pad a multiple of 64.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_conv2d_wino_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int hvpr_conv2d_wino_wgrad_nhwc_f32(const float *x, int N, int H, int W, int Cin, const float *dz, int Cout, float *dw,
                                    void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
size_t hvpr_conv2d_wgrad_workspace_bytes(int N, int OH, int OW, int Cin, int Cout, int taps, int stride);
int hvpr_conv2d_wgrad_nhwc_f32(const float *x, int N, int H, int W, int Cin, const float *dz, int Cout, int taps, int stride, float *dw,
                               void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_conv2d_s2_dgrad_nhwc_f32(const float *dz, int N, int H, int W, int Cin, const float *w_packed, const float *bias, int cout,
                                  int cout_pad, int OH, int OW, float *dx, int out_cstride, int out_coff, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a11 (training)  Train-mode BatchNorm + ReLU over NHWC activations z [P, C] with BATCH statistics — every BatchNorm2d of the
 *     backbone and head, the point stream's shared MLPs and the VFE scale stream.  C % 4 == 0; C <= 1024 for the reductions.
 *     Sums: per-workgroup fp32 partials, final sums in double in a fixed order (deterministic).
 *     hvpr_bn_stats_nhwc_f32: per-channel batch mean, biased variance and 1/sqrt(var + eps) of z.
 *     hvpr_bn_finalize_partials_f32: the same from per-tile sums a producing kernel left behind (hvpr_conv2d_wino_nhwc_f32's
 *         bn_partials [rows][2][C]: sum, sum of squares; count = the pixels they cover).
 *     hvpr_bn_train_affine_f32: what train-mode nn.BatchNorm2d does with the batch moments besides normalising, one launch:
 *         scale = gamma * invstd, shift = beta - mean * scale, and (running_mean / running_var both non-NULL)
 *         running = (1 - momentum) * running + momentum * mean | momentum_unbiased * var (momentum_unbiased = momentum * n / (n - 1)),
 *         *num_batches_tracked += 1 (int64, may be NULL).
 *     hvpr_bn_relu_fwd_nhwc_f32: y = max(0, z * scale + shift) (relu == 0: no max).
 *     hvpr_bn_relu_bwd_sums_nhwc_f32: the LOCAL d gamma = sum dy_m * xhat and d beta = sum dy_m (dy_m = dy through the ReLU / gate).
 *     hvpr_bn_relu_bwd_apply_nhwc_f32: dz (and dgate) of y = relu(gamma * (z - mean) * invstd + beta), the mean / variance terms
 *         differentiated through, from given sums d gamma, d beta and 1 / count.  One rank: _sums, then _apply with its sums and
 *         1 / P.  SyncBatchNorm (tools/train.py:119-120): the caller all-reduces the sums over the ranks between the two and
 *         passes those of the GLOBAL batch with 1 / its count.
 *     gate [P] + resid [P,C] (both or neither; may be NULL): the SFM step fused in, y = gate[p] * relu(...) + resid
 *         (x_att = attention(sfm(x_att), y) + x_att, base_bev_backbone.py:250-255); the backward then also returns dgate [P]
 *         (= sum_c relu(...) * dy, overwritten) and propagates gate * dy; d resid = dy.
 *     Channel slices: y (forward) and dy (backward) are channels [coff, coff + C) of an NHWC tensor with cstride channels per pixel
 *         (cstride % 4 == 0, coff % 4 == 0, coff + C <= cstride; cstride == C, coff == 0: dense).  Every other tensor is dense
 *         [P, C] — resid included.  The backbone's deconvolution branches write straight into the 384-channel concatenation the
 *         head reads and take their gradient out of its gradient.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_bn_workspace_bytes(long long P, int C);
int hvpr_bn_stats_nhwc_f32(const float *z, long long P, int C, float eps, float *mean, float *var, float *invstd, void *workspace,
                           size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_bn_finalize_partials_f32(const float *partials, int rows, int C, long long count, float eps, float *mean, float *var,
                                  float *invstd, hvpr_stream_t stream);
int hvpr_bn_train_affine_f32(const float *mean, const float *var, const float *invstd, int C, const float *gamma, const float *beta,
                             float momentum, float momentum_unbiased, float *running_mean, float *running_var,
                             long long *num_batches_tracked, float *scale, float *shift, hvpr_stream_t stream);
int hvpr_bn_relu_fwd_nhwc_f32(const float *z, long long P, int C, const float *scale, const float *shift, int relu, const float *gate,
                              const float *resid, float *y, int y_cstride, int y_coff, hvpr_stream_t stream);
int hvpr_bn_relu_bwd_sums_nhwc_f32(const float *dy, int dy_cstride, int dy_coff, const float *z, long long P, int C, const float *scale,
                                   const float *shift, const float *mean, const float *invstd, int relu, const float *gate, float *dgamma,
                                   float *dbeta, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_bn_relu_bwd_apply_nhwc_f32(const float *dy, int dy_cstride, int dy_coff, const float *z, long long P, int C, const float *scale,
                                    const float *shift, const float *mean, const float *invstd, int relu, const float *gate, float *dgate,
                                    float *dz, const float *dgamma_total, const float *dbeta_total, double inv_count, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a12 (training)  Anchor target assignment for ONE anchor set (one class of ANCHOR_GENERATOR_CONFIG) and all frames of the batch —
 *     AxisAlignedTargetAssigner.assign_targets_single (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:
 *     113-213; POS_FRACTION < 0: no sampling, NORM_BY_NUM_EXAMPLES false, MATCH_HEIGHT false, as hvpr.yaml:114-124) with
 *     boxes3d_nearest_bev_iou (pcdet/utils/box_utils.py:252-323) and ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:
 *     13-43).  Two launches, no host round trip (the reference: two `.cpu().numpy()` arg-maxes per frame, :148,:153).
 *     MATCH_HEIGHT true (the rotated 3-D IoU as the matcher) and NORM_BY_NUM_EXAMPLES true: the same arguments plus two flags,
 *     hvpr_assign_targets_ex_f32 below.
 *     anchors        [n_anchors, 7] f32 of this set, order (z, y, x, size, rotation); per_loc of them per BEV location
 *     gt_boxes       [batch, n_gt, 8] f32 [x, y, z, dx, dy, dz, heading, class]; trailing rows whose signed sum over the 7 box
 *                    fields (class excluded) is exactly 0 are padding, row 0 is always kept (:53-57, the reference's own rule);
 *                    a row takes part when class_names[class - 1] is this set's class (class_index, 0-based; python's negative
 *                    index for class 0, as the reference has it), n_gt <= 256
 *     outputs in the HEAD's anchor order: entry ((a / per_loc) * loc_stride + loc_offset + a % per_loc) of frame b, rows of
 *     anchors_total entries — loc_stride = anchors per location over all sets, loc_offset = this set's first one:
 *     labels [batch, anchors_total] i32 (-1 don't care, 0 background, class id), reg_targets [batch, anchors_total, 7],
 *     reg_weights [batch, anchors_total] (1 on positives), pos_count [batch] i32 += positives of this set (zero it before the first set).
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_assign_targets_workspace_bytes(int batch, int n_gt);
int hvpr_assign_targets_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int class_index,
                            int n_classes, float matched_thr, float unmatched_thr, int per_loc, int loc_stride, int loc_offset,
                            long long anchors_total, int32_t *labels, float *reg_targets, float *reg_weights, int32_t *pos_count,
                            void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a12 (training)  hvpr_assign_targets_f32 with the two remaining switches of TARGET_ASSIGNER_CONFIG
 *     (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:113-213); every argument up to pos_count, the
 *     trim of padded rows, the class mask, the first maximum over the ground truths, the forced matches, the box code and the
 *     head's anchor order are those of hvpr_assign_targets_f32 above.
 *     match_height          0: boxes3d_nearest_bev_iou, the kernels of hvpr_assign_targets_f32.  non-zero: MATCH_HEIGHT True (:145) —
 *                           the table entry of (anchor, ground truth) is the rotated 3-D IoU, bit for bit what
 *                           hvpr_boxes_pairwise_f32 mode 2 gives for the two rows (the reference's absent native
 *                           boxes_iou3d_gpu).  Two launches: exact rejects on the whole table, the polygon clip on densely packed
 *                           survivors only, once per pass with the same bits; integer atomics only, so labels, targets and
 *                           counts are the same bits on every run.
 *     norm_by_num_examples  non-zero: NORM_BY_NUM_EXAMPLES True (:201-204) — per frame and anchor set n = #(labels >= 0) and
 *                           reg_weights = 1 / max(n, 1) (fp32) on the positives, two small launches more, no host read.  labels,
 *                           reg_targets and pos_count do not depend on it.  The head's losses do not consume reg_weights: they
 *                           rebuild their weights from the labels (anchor_head_template.py:113-119, 190-192), so this flag only
 *                           changes the returned tensor, in the reference as here.
 *     Both 0: the call IS hvpr_assign_targets_f32 (same launches, same bits).  n_gt <= 256; POS_FRACTION sampling is not built.
 *     workspace: hvpr_assign_targets_ex_workspace_bytes(batch, n_gt, n_anchors, match_height) bytes (>= what
 *     hvpr_assign_targets_f32 asks).  After a match_height call its first 8 bytes hold, as one uint64, the number of (anchor,
 *     ground truth) pairs that passed the rejects and were clipped, counted once (pass 1), summed over the frames.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_assign_targets_ex_workspace_bytes(int batch, int n_gt, int n_anchors, int match_height);
int hvpr_assign_targets_ex_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int class_index,
                               int n_classes, float matched_thr, float unmatched_thr, int per_loc, int loc_stride, int loc_offset,
                               long long anchors_total, int32_t *labels, float *reg_targets, float *reg_weights, int32_t *pos_count,
                               int match_height, int norm_by_num_examples, void *workspace, size_t workspace_bytes,
                               hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a12 (training)  TARGET_ASSIGNER_CONFIG.NAME: ATSS — ATSSTargetAssigner.assign_targets for one anchor set and a whole batch
 *     (pcdet/models/dense_heads/target_assigner/atss_target_assigner.py:16-141), written in the head's anchor order like
 *     hvpr_assign_targets_f32: output row (a / per_loc) * loc_stride + loc_offset + a % per_loc of anchors_total, each exactly once.
 *     anchors (n_anchors, 7), gt_boxes (batch, n_gt, 8) with the class in column 7.  Per frame:
 *       - trailing rows whose signed fp32 sum over the 7 box columns is 0 are cut, row 0 never is; NO class mask: every remaining
 *         row of every class takes part;
 *       - the IoU of (anchor, ground truth) is the bits of hvpr_boxes_pairwise_f32 mode 1 (match_height 0) or mode 2 (non-zero);
 *       - candidates of a ground truth: the topk anchors with the smallest 64-bit key (bits of the fp32 squared centre distance
 *         (dx*dx + dy*dy) + dz*dz, then anchor index); thresh = float(mean) + float(std) + 1e-6f of their IoUs, mean and unbiased
 *         variance summed in float64 in key order (topk 1: NaN, nothing positive); a candidate is positive when iou >= thresh
 *         and its centre passes the reference's inside test (rotate by -heading, x against dy / 2, y against dx / 2, closed);
 *       - an anchor takes the ground truth of its highest positive IoU, the lowest row on ties;
 *       - then every ground truth, in ascending order, takes the anchor of its maximum IoU over ALL anchors (lowest index on ties,
 *         anchor 0 where the maximum is 0): no `> 0` guard, the highest row wins a shared anchor;
 *       - labels = class of the matched row (int32; 0 for an unmatched anchor and for a class outside 0 .. n_classes), no -1 band;
 *         reg_targets = ResidualCoder.encode_torch where label > 0, zero elsewhere; reg_weights = 1 / 0; pos_count[frame] +=
 *         #(label > 0) (the caller zeroes it).
 *     n_gt == 0 writes background.  Limits: 1 <= topk <= 64, topk <= n_anchors, n_gt <= 256.  Integer atomics only: the same bytes
 *     on every run; capturable.  workspace: hvpr_assign_targets_atss_workspace_bytes(batch, n_gt, n_anchors, topk) bytes (0 for
 *     arguments the call would refuse).
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_assign_targets_atss_workspace_bytes(int batch, int n_gt, int n_anchors, int topk);
int hvpr_assign_targets_atss_f32(const float *anchors, int n_anchors, const float *gt_boxes, int batch, int n_gt, int n_classes,
                                 int topk, int match_height, int per_loc, int loc_stride, int loc_offset, long long anchors_total,
                                 int32_t *labels, float *reg_targets, float *reg_weights, int32_t *pos_count,
                                 void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a13 (training)  The three losses of ONE prediction stream of the anchor head AND their gradients w.r.t. the predictions, one launch
 *     + a fixed-order sum — get_cls_layer_loss / get_box_reg_layer_loss (pcdet/models/dense_heads/anchor_head_template.py:101-260):
 *     sigmoid focal loss (alpha, gamma = 2; pcdet/utils/loss_utils.py:9-72) with weights 1 / max(#positives of the frame, 1) on
 *     positives and negatives, smooth-L1 (beta) on the sin-difference-encoded residuals (:153-160; loss_utils.py:75-136, NaN targets
 *     ignored), cross entropy on the direction bin of the ground-truth heading (:162-176; loss_utils.py:181-206); each summed over
 *     the batch, / batch, x its LOSS_WEIGHTS entry.
 *     cls_preds [batch, n_anchors, num_class], box_preds [batch, n_anchors, 7], dir_preds [batch, n_anchors, num_dir_bins] or NULL
 *     (NHWC head outputs viewed per anchor); labels / reg_targets / pos_count from hvpr_assign_targets_f32; anchor_rot [n_anchors]
 *     the anchors' headings in the same order; code_weights: 7 floats in HOST memory.
 *     losses [3] (device): cls, loc, dir.  grad_* : d(loss_i)/d(pred), same shapes as the predictions (loss weights and 1 / batch
 *     included: a caller scales them by the upstream gradient of the respective scalar).  num_class <= 3, num_dir_bins <= 8.
 *
 *     hvpr_mse_loss_f32: get_mem_loss (:262-275) — mean((x - target)^2) / rows * weight over [rows, cols] matrices, and its gradient
 *     w.r.t. x (the target is a constant there: `target.detach()`, :268).
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_rpn_losses_workspace_bytes(int batch, long long n_anchors);
int hvpr_rpn_losses_f32(const float *cls_preds, const float *box_preds, const float *dir_preds, const int32_t *labels,
                        const float *reg_targets, const float *anchor_rot, const int32_t *pos_count, int batch, long long n_anchors,
                        int num_class, int num_dir_bins, float alpha, float gamma, float beta, const float *code_weights,
                        float cls_weight, float loc_weight, float dir_weight, float dir_offset, float *losses, float *grad_cls,
                        float *grad_box, float *grad_dir, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
size_t hvpr_mse_loss_workspace_bytes(void);
int hvpr_mse_loss_f32(const float *x, const float *target, long long rows, int cols, float weight, float *loss, float *grad_x,
                      void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a14 (training)  Optimiser step over ONE flat fp32 parameter buffer (and matching flat gradient / moment buffers, all
 *     16-byte aligned): decoupled weight decay p *= 1 - weight_decay * lr, then Adam with bias correction at `step` (1-based)
 *     — OptimWrapper.step, tools/train_utils/optimization/fastai_optim.py:132-149 (true_wd, the optimiser's own weight_decay
 *     forced to 0) around torch.optim.Adam(betas = (beta1, beta2)).  grad_scale_device (may be NULL): a device float every
 *     gradient is multiplied by first — the clip coefficient min(1, clip / (||g|| + 1e-6)) of
 *     clip_grad_norm_ (tools/train_utils/train_utils.py:41), so that clipping costs no extra pass and no host sync.
 * ------------------------------------------------------------------------------------------- */
int hvpr_fused_adam_truewd_f32(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, long long n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int step,
                               const float *grad_scale_device, hvpr_stream_t stream);
/*     The other two optimisers of build_optimizer (tools/train_utils/optimization/__init__.py:12-18) over the same flat buffers,
 *     with the same grad_scale_device and the same argument rules (n == 0: HVPR_OK without a launch; n < 0, a NULL or
 *     misaligned required pointer, step < 1, a beta or momentum outside [0, 1): HVPR_ERR_INVALID_ARG).
 *     hvpr_fused_adam_l2_f32: torch.optim.Adam with COUPLED decay — g' = g * scale + weight_decay * p, then the same Adam step on g'.
 *     hvpr_fused_sgd_f32: torch.optim.SGD with dampening 0 and no Nesterov — d = g * scale + weight_decay * p; with momentum != 0
 *     buf = momentum * buf + d, d = buf; p -= lr * d.  momentum_buf starts zeroed (0 * momentum + d == d is torch's first step, so
 *     there is no step counter); momentum == 0 takes a NULL momentum_buf (one given is neither read nor written). */
int hvpr_fused_adam_l2_f32(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, long long n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step, const float *grad_scale_device,
                           hvpr_stream_t stream);
int hvpr_fused_sgd_f32(float *params, const float *grads, float *momentum_buf, long long n, float lr, float momentum,
                       float weight_decay, const float *grad_scale_device, hvpr_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * a5 / a11  Stride-1 3x3 convolution (pad 1) by Winograd F(2x2, 3x3) on the fp32 matrix cores: the same operation as
 *     hvpr_conv2d_nhwc_f32 with taps = 9, stride = 1, up = 1 — BaseBEVBackbone_Scale's Conv3x3 + BN + ReLU and the SFM step
 *     (pcdet/models/backbones_2d/base_bev_backbone.py:228-315) — with 16 instead of 36 fp32 multiplies per 2x2 output block and
 *     (cin, cout) pair.  All arithmetic is fp32; the result differs from the direct kernel by summation order only
 *     (observed <= 2e-6 relative to the output scale per layer, tests/test_gpu_conv_wino.py).
 *
 *     hvpr_conv2d_wino_pack_f32: weight [cout, cin, 3, 3] f32 (torch OIHW), optional per-output-channel scale [cout] (folded
 *         BatchNorm), -> packed [hvpr_conv2d_wino_packed_floats(cin, cout)] f32 = U = G g Gt in the kernel's stage image
 *         [cout_pad/64][cin/8][16][2][64][4] (cout_pad = cout rounded up to 64; transform evaluated in double, rounded once).
 *         adjoint != 0: `weight` is the [cin, cout, 3, 3] filter of the layer whose DATA GRADIENT is wanted: packs
 *         w'[o][i][u][v] = weight[i][o][2-u][2-v].
 *     hvpr_conv2d_wino_nhwc_f32: in [N,H,W,Cin] (Cin % 8 == 0), bias [cout_pad], gate / resid / out / out_cstride / out_coff as
 *         in hvpr_conv2d_nhwc_f32 (cout % 4 == 0).  px_groups: 1 = 8 x 16 output pixels x 64 channels per workgroup (4 waves),
 *         2 = 16 x 16 pixels x 64 channels (8 waves sharing the filter stage), 4 = 8 x 16 pixels x 32 channels (4 waves; twice
 *         the tiles for launches that do not fill the chip).  With px_groups == 1 and no bn_partials, ragged edge tiles are
 *         paired: where the last tile column has at most 4 live 2x2-block columns, the right-edge tiles of tile rows 2r and
 *         2r + 1 are one workgroup item, and where the last tile row has at most 2 live block rows, so are bottom-edge tiles 2c
 *         and 2c + 1 (csrc/wino_walk.h).  The result is bit-identical to the unpaired walk.
 *     hvpr_conv2d_wino_items: the number of workgroup items (pixel tiles or tile pairs, times channel tiles) that launch walks;
 *         px_groups == 1 describes the launch without bn_partials (the statistics launch walks hvpr_conv2d_wino_stats_rows x
 *         cout_pad / 64 items).  0 for invalid arguments.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_conv2d_wino_packed_floats(int cin, int cout);
int hvpr_conv2d_wino_pack_f32(const float *weight, const float *scale, int cout, int cin, int adjoint, float *packed,
                              hvpr_stream_t stream);
int hvpr_conv2d_wino_nhwc_f32(const float *in, int N, int H, int W, int Cin, const float *w_packed, const float *bias, int cout,
                              int relu, const float *gate, const float *resid, int resid_cstride, float *out, int out_cstride,
                              int out_coff, int px_groups, float *bn_partials, hvpr_stream_t stream);
/* bn_partials (optional, training): [hvpr_conv2d_wino_stats_rows(N, H, W)][2][cout] f32, overwritten with the per-pixel-tile sum
 * and sum of squares of the raw output (px_groups == 1, relu == 0, no gate) — the batch statistics of the layer's BatchNorm without
 * a pass over the written tensor; hvpr_bn_finalize_partials_f32 turns them into mean / biased variance / 1/sqrt(var + eps)
 * (count = N * H * W; sums finished in double, fixed order: deterministic). */
int hvpr_conv2d_wino_stats_rows(int N, int H, int W);
int hvpr_conv2d_wino_items(int N, int H, int W, int cout, int px_groups);
/* Walk table of the px_groups == 1 launch without bn_partials, as for hvpr_conv2d_nhwc_tab_f32: hvpr_conv2d_wino_tab_bytes bytes (0
 * for every other px_groups: no table) filled once per (N, H, W, cout) by hvpr_conv2d_wino_tab_build, one 8-byte entry per walk step
 * (hvpr_conv2d_wino_items rounded up to whole rounds of 8 pixel items: csrc/wino_walk.h); hvpr_conv2d_wino_nhwc_tab_f32 is
 * hvpr_conv2d_wino_nhwc_f32 with `table` = that table or NULL (the in-kernel decode), bit-identical either way. */
size_t hvpr_conv2d_wino_tab_bytes(int N, int H, int W, int cout, int px_groups);
int hvpr_conv2d_wino_tab_build(int N, int H, int W, int cout, int px_groups, void *table, hvpr_stream_t stream);
int hvpr_conv2d_wino_nhwc_tab_f32(const float *in, int N, int H, int W, int Cin, const float *w_packed, const float *bias, int cout,
                                  int relu, const float *gate, const float *resid, int resid_cstride, float *out, int out_cstride,
                                  int out_coff, int px_groups, float *bn_partials, const void *table, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a5 optional precision modes: 3x3 convolutions on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulation)
 *     with split operands.  n_planes = 2 ("bf16x3"): x = hi + lo, x*w ~= hi*hi + hi*lo + lo*hi, error ~2^-16 relative per
 *     product — SURVEY.md §8d allows a reduced-precision path evidenced within the 1e-3 tolerance.  n_planes = 3 ("bf16x6"):
 *     x = hi + mid + lo exactly, six products, dropped terms <= 2^-23 relative = the accuracy of the fp32 matrix-core kernel
 *     (fp32 emulation).  hvpr_conv2d_nhwc_f32 stays the parity reference.
 *     Split-bf16 NHWC: each group of 8 channels of a pixel is n_planes x [8 x bf16] (16 bytes per plane).
 *     hvpr_split_bf16_f32 / hvpr_unsplit_bf16_f32: fp32 NHWC (n_floats % 8 == 0) <-> split-bf16 NHWC.
 *     hvpr_conv2d_nhwc_bf16x3: in_split [N,H,W,Cin] split, w_split [9, Cin/8, n_planes, cout_pad] x 16 B, bias [cout_pad] f32;
 *     out fp32 NHWC (out_split = 0) or split NHWC (1) with out_cstride channels at channel offset out_coff; optional fused
 *     y = gate*y + resid with resid in split form.  Cin % 16 == 0, cout % 4 == 0, strides/offsets % 8 == 0.
 *     tile_cfg 0 = 128 px x 64 ch, 1 = 64 px x 64 ch, 2 = 256 px x 64 ch (stride 1, two planes); three planes: stride 1 only.
 * ------------------------------------------------------------------------------------------- */
int hvpr_split_bf16_f32(const float *src, long long n_floats, int n_planes, void *dst, hvpr_stream_t stream);
int hvpr_unsplit_bf16_f32(const void *src, long long n_floats, int n_planes, float *dst, hvpr_stream_t stream);
int hvpr_conv2d_nhwc_bf16x3(const void *in_split, int N, int H, int W, int Cin, const void *w_split, const float *bias,
                            int stride, int cout, int cout_pad, int relu, const float *gate, const void *resid_split,
                            int resid_cstride, void *out, int out_split, int out_cstride, int out_coff, int tile_cfg,
                            int n_planes, hvpr_stream_t stream);
/* ConvTranspose2d(kernel = stride = up)+BN+ReLU of the same modes (base_bev_backbone.py:177-188): split input, w_split
 * [1, Cin/8, n_planes, cout_pad] x 16 B with gemm column (ky*up + kx)*cout + co, fp32 output written into channels
 * [out_coff, out_coff + cout) of an NHWC tensor of out_cstride channels at up x the resolution.  Cin % 64 == 0. */
int hvpr_deconv_nhwc_bf16x3(const void *in_split, int N, int H, int W, int Cin, const void *w_split, const float *bias, int cout,
                            int cout_pad, int up, int relu, float *out, int out_cstride, int out_coff, int n_planes,
                            hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f2 ("next" row)  KITTI point pre-processing in front of the voxelizer, on the device.
 *     hvpr_point_flags_f32  mode 0: mask_points_by_range (pcdet/utils/common_utils.py:59-62: x,y in [lo,hi] inclusive;
 *                           range_xy = {x0,y0,x1,y1}) AND, when the two fov matrices are given, KittiDataset.get_fov_flag
 *                           (pcdet/datasets/kitti/kitti_dataset.py:100-116; fov_lidar_to_rect = (V2C^T R0^T) [4][3],
 *                           fov_rect_to_img = P2^T [4][3], both row-major float32 as calibration_kitti.py:65-84 forms them);
 *                           mode 1: the near flag of DataProcessor.sample_points (data_processor.py:89-90): |xyz| < near_thresh.
 *                           points [n, stride] f32 with x,y,z in columns 0..2; flags [n] u8.
 *     hvpr_compact_rows_f32 dst = src[flags != 0] (stable), *count = number of rows (clamped to capacity).
 *     hvpr_gather_rows_f32  dst[r] = src[idx[r]] (points[choice] of sample_points; idx i32, out-of-range rows are zeros).
 * ------------------------------------------------------------------------------------------- */
int hvpr_point_flags_f32(const float *points, int n, int stride, int mode, const float *range_xy, float near_thresh,
                         const float *fov_lidar_to_rect, const float *fov_rect_to_img, int img_h, int img_w, uint8_t *flags,
                         hvpr_stream_t stream);
size_t hvpr_compact_workspace_bytes(int n);
int hvpr_compact_rows_f32(const float *src, int n, int row_floats, const uint8_t *flags, float *dst, int capacity,
                          int32_t *count, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_gather_rows_f32(const float *src, int n_src, int row_floats, const int32_t *idx, int m, float *dst,
                         hvpr_stream_t stream);
/* frame_offsets [batch+1] i32 of a collated point array (dataset.py:161-166: column 0 = batch index, frames contiguous and
 * ascending): offsets[b] = first row of frame b (empty frames included), offsets[batch] = n_points. */
int hvpr_frame_offsets_f32(const float *points, int n_points, int point_stride, int batch, int32_t *frame_offsets,
                           hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f4  Training augmentation on the device, a whole batch per call: GT sampling (database_sampler.py:118-200), world flip /
 *     rotation / scaling (augmentor_utils.py:6-78), limit_period (data_augmentor.py:95-97) and the training-only box trim
 *     (data_processor.py:24-28).  The random draws are the host's; they arrive as one packed plan of 32-bit words (layout:
 *     csrc/augment.hip; packed by hvpr_amd/augment.py), given twice: `plan_host` (read and checked here, before any launch) and
 *     `plan_dev` (the same words on the device, read by the kernels).  Every check is made on the host: a refused call returns
 *     HVPR_ERR_INVALID_ARG / HVPR_ERR_UNSUPPORTED / HVPR_ERR_WORKSPACE and launches nothing, so no output is touched.  No entry
 *     point synchronises or reads the device.
 *     hvpr_augment_collide_f32  valid[c] = 1 when candidate c may be pasted: max IoU against the frame's existing boxes (ALL its
 *                           ground truths, then what earlier groups accepted) plus max IoU against the other candidates of its
 *                           group is exactly 0 (:184-188; an empty existing set takes the group table twice, :187).  The IoU is
 *                           the rotated-BEV routine of hvpr_boxes_pairwise_f32.  A frame may hold 256 ground truths + candidates
 *                           (else HVPR_ERR_UNSUPPORTED).
 *     hvpr_augment_boxes_f32    gt_out [B, g_cap, 8]: per frame the ground truths of trained classes in order, then the accepted
 *                           candidates in order; each row flipped / rotated / scaled, heading through limit_period(., 0.5, 2 pi),
 *                           column 7 = class index + 1; with remove_outside, rows with none of their 8 corners inside range6
 *                           (x0 y0 z0 x1 y1 z1, a HOST pointer, bounds inclusive) are dropped (box_utils.py:55-71); rows are compacted
 *                           stably, zero rows follow, box_count[f] rows are live.  g_cap must hold every frame's rows even if all
 *                           its candidates were accepted.
 *     hvpr_augment_points_f32   out_points / out_off [B+1] i32: per frame the accepted candidates' points in candidate order (bank
 *                           arena rows + the object's database box centre, z minus the road-plane move), then the scene points
 *                           that lie in no accepted candidate's box enlarged by extra_width3 (a HOST pointer; inside means
 *                           |z - cz| <= dz/2, |x| < dx/2 and |y| < dy/2 in the box frame), in their order; every written point is
 *                           flipped / rotated / scaled, the other features pass through.  The rotation of a point is x' = fmaf(y, -s, x c),
 *                           y' = fmaf(y, c, x s): the second product fused, as the reference's float32 gemm over a frame's points
 *                           accumulates; a box row (hvpr_augment_boxes_f32) takes the unfused sum of torch's small-matrix path.  Count pass, one-workgroup scan, write
 *                           pass: no atomics, stable, bit-reproducible.  out_capacity (rows) must be at least n_points + the
 *                           points of ALL candidates; bank_floats must equal point_floats; candidate object ids must lie in
 *                           [0, n_objects) and their rows inside bank_rows; 256 candidates per frame; rows are 32-bit offsets.
 *     hvpr_augment_block_points scene points per workgroup of the count / write passes (tests put frame sizes around it).
 * ------------------------------------------------------------------------------------------- */
int hvpr_augment_block_points(void);
int hvpr_augment_collide_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, int32_t *valid,
                             hvpr_stream_t stream);
int hvpr_augment_boxes_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, const int32_t *valid,
                           const float *range6, int remove_outside, int g_cap, float *gt_out, int32_t *box_count,
                           hvpr_stream_t stream);
size_t hvpr_augment_points_workspace_bytes(int n_frames, int max_frame_points, int n_candidates, long long n_points);
int hvpr_augment_points_f32(const int32_t *plan_host, const int32_t *plan_dev, int plan_words, const int32_t *valid,
                            const float *points, long long n_points, int point_floats, const float *bank_points,
                            long long bank_rows, const float *bank_boxes, int n_objects, int bank_floats,
                            const float *extra_width3, float *out_points, long long out_capacity, int32_t *out_off,
                            void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f6  The GT-sampling database from raw frames, a chunk of frames per call: the loop of KittiDataset.
 *     create_groundtruth_database (kitti_dataset.py:205-238).  A chunk is one ragged point array `points` [n_points,
 *     point_floats] f32 (3 <= point_floats <= 8, x y z first) with `pt_off` [n_frames + 1] i32, and the frames' annotated boxes
 *     `boxes` [n_obj, 7] f32 (x y z dx dy dz heading) with `box_off` [n_frames + 1] i32.  Both offset arrays are given twice: the
 *     `_host` copy is read and checked here, before any launch, the other is the same words on the device, read by the kernels.
 *     Every check is made on the host: a refused call returns HVPR_ERR_INVALID_ARG / HVPR_ERR_UNSUPPORTED / HVPR_ERR_WORKSPACE
 *     and launches nothing, so no output is touched.  No entry point synchronises or reads the device.  A frame may hold 256
 *     boxes and a chunk 65535 frames (else HVPR_ERR_UNSUPPORTED); rows are 32-bit offsets.
 *     A point is inside a box when |z - cz| <= dz/2 and, turned by -heading about the centre, |x| < dx/2 and |y| < dy/2: the
 *     fp32 operations of hvpr_points_in_boxes_cpu (include/hvpr_cpu.h) in their order.
 *     hvpr_gt_database_count_f32    obj_count[k] = points of box k's frame inside box k.  Per box and block of scene points the
 *                           count stays in `workspace` for the extract call.  Usable alone, as the count-only mode.
 *     hvpr_gt_database_extract_f32  after the host has read obj_count (`obj_count_host`, checked against `arena_capacity` rows:
 *                           their sum must fit) and with the workspace the count call of the SAME chunk filled: obj_off
 *                           [n_obj + 1] i32 = the exclusive prefix of obj_count, and arena rows obj_off[k] .. obj_off[k+1] = box
 *                           k's points in the ascending order they have in their frame (a point inside two boxes appears in
 *                           both).  Columns 0..2 are (float)((double)p - centres[k]) with `centres` [n_obj, 3] f64: numpy's
 *                           float32 array minus float64 box (:226) rounds once; the other columns are copied.  Count pass,
 *                           scans, write pass: no atomics, stable, bit-reproducible.  A row at or past arena_capacity is never
 *                           written, whatever the device counts hold.
 *     hvpr_gt_database_workspace_bytes  for frames of at most max_frame_points points and n_obj boxes in all; 0 for an empty
 *                           chunk.  Needs no GPU.
 *     hvpr_gt_database_block_points scene points per workgroup of the count / write passes (tests put frame sizes around it).
 * ------------------------------------------------------------------------------------------- */
int hvpr_gt_database_block_points(void);
size_t hvpr_gt_database_workspace_bytes(int n_frames, int max_frame_points, int n_obj);
int hvpr_gt_database_count_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                               const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                               const int32_t *box_off, int n_obj, int32_t *obj_count, void *workspace, size_t workspace_bytes,
                               hvpr_stream_t stream);
int hvpr_gt_database_extract_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                                 const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                                 const int32_t *box_off, const double *centres, int n_obj, const int32_t *obj_count_host,
                                 const int32_t *obj_count, int32_t *obj_off, float *arena, long long arena_capacity,
                                 void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f7  Training batches on the device: ragged select / shuffle / collate, a whole batch per call (get_fov_flag,
 *     mask_points_by_range, shuffle_points and the `points` branch of collate_batch).  The frames lie end to end in `points`
 *     [rows, point_floats] f32 (3 <= point_floats <= 64, x y z first) with DEVICE-resident offsets `off` [n_frames + 1] i32,
 *     ascending; rows at or past off[n_frames] are capacity and are ignored, and an offset outside [0, rows] is clamped into
 *     it, so no row outside the array is ever read.  n_frames <= 1024, rows are 32-bit offsets (else HVPR_ERR_UNSUPPORTED).
 *     `mask` picks the decision: bit 1 (value 1) the FOV test with the frame's row of `calib` [n_frames, 26] f32 on the device
 *     (the layout of eval_loop.pack_calib: V2C^T R0^T 4x3, P2 3x4, image height, image width), bit 2 (value 2) the x/y range
 *     `range_xy` (4 HOST floats x0 y0 x1 y1, both ends inclusive); both bits: the AND; 0 keeps every row in front of off[B].
 *     The fp32 operations are those of hvpr_point_flags_f32 mode 0 in their order (one shared expression): the same decisions.
 *     Every check is made on the host: a refused call returns HVPR_ERR_INVALID_ARG / HVPR_ERR_UNSUPPORTED /
 *     HVPR_ERR_WORKSPACE and launches nothing.  No entry point synchronises or reads the device.
 *     hvpr_ragged_select_count_f32  new_off [n_frames + 1] i32: new_off[b] = kept rows in front of off[b] (new_off[0] = 0), the
 *                           offsets of the compacted batch.  Per-tile counts and their prefix stay in `workspace` for the
 *                           write call of the SAME input.  Usable alone.
 *     hvpr_ragged_select_write_f32  the kept rows, stable.  The kept row of flat rank r (0-based among all kept rows) in frame b
 *                           goes to output row r, or with `inv_perm` [n_perm] i32 (flat, indexed by r) to row
 *                           new_off[b] + inv_perm[r]: out[new_off[b] + i] = compacted_b[perm_b[i]] for inv_perm = the
 *                           inverse of perm_b.  batch_column != 0 writes (float)b in front of the row: `out` is
 *                           [out_capacity, point_floats + 1], else [out_capacity, point_floats].  A row whose inv_perm
 *                           entry is outside [0, new_off[b+1] - new_off[b]), whose rank is at or past n_perm, or whose
 *                           destination is at or past out_capacity is dropped and sets *flag = 1 (a device word the caller
 *                           zeroes): nothing is ever written outside `out`.
 *     Count pass, one-workgroup scan, write pass: no atomics, stable, bit-reproducible.
 *     hvpr_ragged_select_workspace_bytes  for an array of `rows` rows and n_frames frames.  Needs no GPU.
 *     hvpr_ragged_select_tile_rows  rows per workgroup of the count / write passes (tests put frame sizes around it).
 * ------------------------------------------------------------------------------------------- */
int hvpr_ragged_select_tile_rows(void);
size_t hvpr_ragged_select_workspace_bytes(long long rows, int n_frames);
int hvpr_ragged_select_count_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                 int mask, const float *calib, const float *range_xy, int32_t *new_off, void *workspace,
                                 size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_ragged_select_write_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                 int mask, const float *calib, const float *range_xy, const int32_t *new_off,
                                 const int32_t *inv_perm, long long n_perm, int batch_column, float *out,
                                 long long out_capacity, int32_t *flag, void *workspace, size_t workspace_bytes,
                                 hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f7b DataProcessor.sample_points for a whole batch, fused into the select / shuffle / collate above (same input layout, same
 *     `mask`, same limits and refusals).  The reference's draws depend on a frame only through n, its kept rows, and c, its
 *     kept rows with ||xyz||_2 < `near` (the expression of hvpr_point_flags_f32 mode 1, one shared copy; near >= 0): the host
 *     reads both counts, draws over ordinals and hands back where every kept row goes.
 *     hvpr_ragged_sample_count_f32  new_off as hvpr_ragged_select_count_f32 gives it, bit for bit, and near_off
 *                           [n_frames + 1] i32: near_off[b] = kept-and-near rows in front of off[b].  Per-tile counts and
 *                           prefixes of both stay in `workspace` for the write call of the SAME input.
 *     hvpr_ragged_sample_write_f32  for a kept row of frame b with in-frame rank r (among the frame's kept rows) and near
 *                           ordinal a (kept-and-near rows of the frame in front of it), c = the frame's near count: the
 *                           source ordinal s is r when mode[b] == 0; when mode[b] == 1 it is a for a near row and
 *                           c + (r - a) for a far one (near ordinals first, then the far ones, both ascending).  `mode`
 *                           [n_frames] i32 and `dest` [n_dest, 2] i32 (8-byte aligned) are on the device; the row's two
 *                           destinations are dest[new_off[b] + s][0..1], -1 for none, and for each d >= 0 the row is stored
 *                           at out[b * num_points + d], with (float)b in front when batch_column != 0.  A destination
 *                           outside [-1, num_points), a table index at or past n_dest, an output row at or past
 *                           out_capacity or a mode other than 0 / 1 drops the store and sets *flag = 1 (a device word the
 *                           caller zeroes): nothing is ever written outside `out`.  Output rows no entry names stay as
 *                           they were.
 *     No atomics, no flag array, no spin-waits: the same input gives the same bytes.
 *     hvpr_ragged_sample_workspace_bytes  for both calls (twice the layout of hvpr_ragged_select_workspace_bytes).  Needs no GPU.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_ragged_sample_workspace_bytes(long long rows, int n_frames);
int hvpr_ragged_sample_count_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                 int mask, const float *calib, const float *range_xy, float near, int32_t *new_off,
                                 int32_t *near_off, void *workspace, size_t workspace_bytes, hvpr_stream_t stream);
int hvpr_ragged_sample_write_f32(const float *points, long long rows, int point_floats, const int32_t *off, int n_frames,
                                 int mask, const float *calib, const float *range_xy, float near, const int32_t *new_off,
                                 const int32_t *near_off, const int32_t *mode, const int32_t *dest, long long n_dest,
                                 int num_points, int batch_column, float *out, long long out_capacity, int32_t *flag,
                                 void *workspace, size_t workspace_bytes, hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f8  get_infos' num_points_in_gt, a chunk of frames per call: the loop of KittiDataset.get_infos (kitti_dataset.py:171-184).
 *     The chunk is f6's: `points` [n_points, point_floats] f32 (3 <= point_floats <= 8) with `pt_off`, `boxes` [n_obj, 7] f32
 *     with `box_off`, both offset arrays [n_frames + 1] i32 given twice (`_host` read and checked here, the other read by the
 *     kernels), a frame of at most 256 boxes, a chunk of at most 65535 frames, 32-bit rows.  The calibration table is f7's:
 *     `calib` [n_frames, 26] f32 (eval_loop.pack_calib: V2C^T R0^T 4x3, P2 3x4, image height, image width), also given twice;
 *     the host copy is checked for image height and width > 0.  Every check is made on the host: a refused call returns
 *     HVPR_ERR_INVALID_ARG / HVPR_ERR_UNSUPPORTED / HVPR_ERR_WORKSPACE and launches nothing.  The call only enqueues.
 *     hvpr_kitti_infos_count_f32    obj_count[k] = points of box k's frame that are in that frame's camera view AND inside box
 *                           k.  The view test is the shared expression of hvpr_point_flags_f32 mode 0 and the ragged select
 *                           (the same decisions, bit for bit); the box test is f6's (the hull of a cuboid's corners is the
 *                           cuboid; on a face `<=` / `<` decide here and Qhull's tolerance in the reference: unpinned; a box
 *                           with a zero size counts 0).  `fov_count` [n_frames] i32, or NULL to skip it: the frame's points in
 *                           view.  With n_obj == 0 and fov_count NULL nothing is launched.  No atomics, bit-reproducible.
 *     hvpr_kitti_infos_workspace_bytes  for frames of at most max_frame_points points and n_obj boxes in all (per box and per
 *                           frame one partial count per block); 0 for a chunk without frames.  Needs no GPU.
 *     hvpr_kitti_infos_block_points scene points per workgroup: the block of hvpr_gt_database_block_points, the same number.
 * ------------------------------------------------------------------------------------------- */
int hvpr_kitti_infos_block_points(void);
size_t hvpr_kitti_infos_workspace_bytes(int n_frames, int max_frame_points, int n_obj);
int hvpr_kitti_infos_count_f32(const float *points, long long n_points, int point_floats, const int32_t *pt_off_host,
                               const int32_t *pt_off, int n_frames, const float *boxes, const int32_t *box_off_host,
                               const int32_t *box_off, int n_obj, const float *calib_host, const float *calib,
                               int32_t *obj_count, int32_t *fov_count, void *workspace, size_t workspace_bytes,
                               hvpr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * v1  The bird's-eye-view picture of a batch: tools/vis.py kitti_vis (:279-286) -- point_to_vis_bev (:109-121) over points_to_bev /
 *     _points_to_bevmap_reverse_kernel (:9-106) with ONE height slice, then draw_box_in_bev (:223-249) -- for every frame of a
 *     batch in one call, from the forms the batch loader and post_processing(sync=False) leave on the device.
 *     points        [n_points, point_stride] f32, xyz at columns xyz_col..xyz_col+2 (the loader's batch column costs no copy);
 *                   frame_offsets [batch + 1] i32 on the device: frame b owns rows offsets[b] .. offsets[b + 1] - 1; a row no
 *                   frame owns and a point with a non-finite coordinate are dropped.
 *     range, pixel  range[6] f32 on the HOST (x, y, z low, then high), read during the call; the grid is W = round((hi_x - lo_x) /
 *                   pixel), H = round((hi_y - lo_y) / pixel) in float32 with ties to even, as points_to_bev forms it; the one
 *                   height slice is range[5] - range[2] (float32) high.
 *     height pass   a point belongs to cell floor((p - lo) / size) per axis in float32 (a true division) and is dropped when that
 *                   is < 0 or >= the grid, z included; a cell's value is the maximum over its points of (z - z_lo) / (z_hi - z_lo)
 *                   formed in double and rounded to float32, from 0; `counts` [batch, H, W] i32 (or NULL) is bev_map[-1], the
 *                   points per cell.  Integer atomics only (max on the bits of a float >= 0, add): bit-reproducible.
 *                   UNPINNED: the reference's loop ends at the max_voxels-th (80 000) newly opened cell in point order; this op has
 *                   no such cap.
 *     box tables    two, each optional (boxes NULL): boxes [batch, rows, box_stride] f32 with x, y, z, dx, dy, dz, heading in the
 *                   first 7 floats of a row (box_stride >= 7); count [batch] i32 or NULL: only the first count[b] rows of frame b;
 *                   scores [batch, rows] f32 or NULL: a row is drawn when score >= thresh; labels [batch, rows] i64 or NULL.  A
 *                   row's ink is `ink` + its label (`ink` alone without labels); a row whose ink is < 1 or >= n_ink, or with a
 *                   non-finite field, is not drawn.  palette [n_ink, 3] u8 on the device; ink 0 is "nothing drawn".
 *     box pass      center_to_corner_box2d's corners in float32 (rotation_2d turns CLOCKWISE for a positive angle), plus the
 *                   centre, minus range[:2], times (W, H) / (hi - lo)[:2] (both steps in float64, each rounded to float32, as
 *                   numpy's in-place updates do), truncated toward zero and clamped to +-8191.  Per box the reference's THREE
 *                   segments, corners 0-1, 2-3, 3-0 (bev_lines, :244-246; the edge 1-2 is left open there too).  heading_sign +1
 *                   draws a lidar box (counter-clockwise heading) mirrored, as the reference does; -1 negates the angle first and
 *                   is the correct drawing.
 *                   UNPINNED: cv2.line's rasterisation.  The rule here: pixel p takes a segment's ink when 4 d^2 <= thickness^2, d
 *                   the distance from p to the integer segment, evaluated exactly in int64 (at thickness 1 this contains every
 *                   Bresenham pixel).  Where inks meet the larger index wins (integer atomic max), on every run.
 *     image         [batch, H, W, 3] u8: the ink's palette row where ink was drawn, else uint8(v * 255) (float32 product) in all
 *                   three channels.
 *     Refusals, before any launch: HVPR_ERR_INVALID_ARG for a null frame_offsets / range / image / palette / workspace (or points
 *     with n_points > 0), batch < 1, n_ink < 1, thickness < 1, heading_sign other than +-1, xyz_col outside the row, a
 *     non-finite or empty range, pixel <= 0, a table with rows < 0 or box_stride < 7; HVPR_ERR_UNSUPPORTED for W or H > 8192,
 *     thickness > 255, batch > 65535, batch * H * W or n_points >= 2^31, a table of more than 2^20 rows; HVPR_ERR_WORKSPACE.
 *     Four launches at most, no host read, no allocation: capturable into a hipGraph.
 *     hvpr_render_bev_workspace_bytes  for [batch, height, width] pixels (three 32-bit planes); 0 for a shape that is refused.
 *                   Needs no GPU.
 * ------------------------------------------------------------------------------------------- */
size_t hvpr_render_bev_workspace_bytes(int batch, int height, int width);
int hvpr_render_bev_u8(const float *points, long long n_points, int point_stride, int xyz_col, const int32_t *frame_offsets,
                       int batch, const float *range, float pixel, const float *boxes0, int rows0, int box_stride0,
                       const int32_t *count0, const float *scores0, float thresh0, const long long *labels0, int ink0,
                       const float *boxes1, int rows1, int box_stride1, const int32_t *count1, const float *scores1,
                       float thresh1, const long long *labels1, int ink1, const uint8_t *palette, int n_ink, int thickness,
                       int heading_sign, uint8_t *image, int32_t *counts, void *workspace, size_t workspace_bytes,
                       hvpr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HVPR_AMD_H */
