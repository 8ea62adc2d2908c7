/*
 * toda.h — C ABI of libtoda_hip.so, the MI355X (gfx950) implementation of the
 * sparse LiDAR-detection hot path of rasd3/TODA (an OpenPCDet fork).
 *
 * The reference reaches this arithmetic through the third-party `spconv`
 * package (not vendored, not pinned).  Every entry point below names the
 * reference call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *     small geometry arrays (range, vsize, shape, ksize, ...) are HOST arrays
 *     read during the call.
 *   - the caller owns all memory, including workspaces; nothing here allocates
 *     or frees device memory and nothing synchronises the device.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *   - return value: 0 on success, a negative TODA_E* code on failure; the
 *     message is available from toda_last_error() (thread local).
 *   - sizes that live on the device (`*_dev`) are int32 scalars; a kernel that
 *     takes both `n` and `n_dev` uses min(n, *n_dev) rows when n_dev != NULL,
 *     so index-building phases can be chained without a host round trip.
 *   - indices are int32 rows of (b, z, y, x); spatial shapes are (D, H, W).
 *   - neighbour tables are k-major: nbr[k * n_rows + row], -1 = no neighbour,
 *     k = (kz * KY + ky) * KX + kx.
 *   - weights use the spconv-2 layout [Cout][kz][ky][kx][Cin]
 *     (pcdet/models/detectors/detector3d_template.py:337-348 converts v1 layouts).
 */
#ifndef TODA_H_
#define TODA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TODA_OK 0
#define TODA_EINVAL (-1)   /* bad argument / unsupported shape            */
#define TODA_EWORKSPACE (-2) /* workspace too small                       */
#define TODA_ELAUNCH (-3)  /* HIP launch or runtime error                 */
#define TODA_EFAULT (-4)   /* a kernel reported a fault (toda_device_fault) */

/* Bits of the device fault word: the kernels whose workgroups wait for each other inside one launch bound their spins;
 * a wait that gives up raises its bit and the launch finishes with invalid numbers instead of hanging the GPU. */
#define TODA_FAULT_BN2D 1u /* bn2d_fwd/bwd_kernel<V, 0, K, RELU> (one workgroup per plane): partner never published */
#define TODA_FAULT_WINO 2u /* wino_fwd_ws_kernel: stream-K contributor never published */
#define TODA_FAULT_FPS 4u  /* fps_multi_kernel: a workgroup of the sample's group never arrived */

const char* toda_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int toda_abi_version(void);
/* Reads and clears the fault word (host-mapped memory: no device synchronisation).  TODA_OK, or TODA_EFAULT with the
 * kernels named in toda_last_error().  toda_bn2d_* and toda_conv3x3_fwd poll it on entry as well, so a fault raised by
 * one launch is reported by the next call of that family at the latest; call it after a synchronisation point to learn
 * about the launches before it.  (No reference counterpart: the reference's cuDNN / spconv kernels never wait on each other.) */
int toda_device_fault(void);

/* ------------------------------------------------------------------------
 * Hard voxelisation.  Replaces spconv Point2VoxelCPU3d.point_to_voxel /
 * VoxelGenerator.generate as called from
 * pcdet/datasets/processor/data_processor.py:44-60,115-143.
 * Sequential semantics (voxel ids in order of first appearance, first
 * `max_pts` points kept per voxel, voxels past `max_voxels` dropped) are
 * reproduced exactly.  `points` is [n, c] fp32, xyz in columns 0..2.
 * Outputs sized for max_voxels: voxels [max_voxels, max_pts, c] (zero padded
 * for rows < *m_dev), coords_zyx [max_voxels, 3], num_pts [max_voxels].
 * ---------------------------------------------------------------------- */
size_t toda_voxelize_workspace_bytes(int n_points, int max_voxels);
int toda_voxelize_hard(const float* points, int n, int c,
                       const float* range_host /*[6] x0 y0 z0 x1 y1 z1*/,
                       const float* vsize_host /*[3] xyz*/,
                       const int32_t* grid_host /*[3] xyz cells*/,
                       int max_pts, int max_voxels,
                       float* voxels, int32_t* coords_zyx, int32_t* num_pts,
                       int32_t* m_dev, void* ws, size_t ws_bytes, void* stream);
/* The same for a whole batch in three launches: the per-sample voxelisation of the DataLoader workers
 * (data_processor.py:115-143) AND collate_batch's concatenation with the batch column prepended
 * (pcdet/datasets/dataset.py:161-178).  points_host[b] is the DEVICE address of sample b's first feature
 * column, rows `row_stride` floats apart (a [sum N, 1 + C] batch tensor is read in place: address of column 1,
 * stride 1 + C); n_points_host[b] <= n_cap, the per-sample capacity the workspace is laid out for.  Outputs
 * are the collated tensors, samples back to back, each clipped at max_voxels: voxels [sum M_b, max_pts, c],
 * coords_bzyx [sum M_b, 4], num_pts [sum M_b]; room for batch * min(max_voxels, n_cap) rows.
 * counts_dev [batch + 1] = M_0 .. M_{batch-1}, sum M_b.  ws_clean != 0: the workspace was used by this entry
 * point before with the same (batch, n_cap) - every call leaves its hash table empty - and nothing else wrote it;
 * 0: the call clears the table first.  After a failed call pass 0. */
size_t toda_voxelize_batch_workspace_bytes(int batch, int n_cap);
int toda_voxelize_batch(const float* const* points_host, const int32_t* n_points_host, int batch, int n_cap,
                        int c, int row_stride,
                        const float* range_host, const float* vsize_host, const int32_t* grid_host,
                        int max_pts, int max_voxels,
                        float* voxels, int32_t* coords_bzyx, int32_t* num_pts, int32_t* counts_dev,
                        void* ws, size_t ws_bytes, int ws_clean, void* stream);

/* MeanVFE: pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31.
 * out[v, :] = sum_p voxels[v, p, :] / max(num_pts[v], 1); num_pts is fp32
 * because load_data_to_gpu (pcdet/models/__init__.py:23-34) casts it. */
int toda_mean_vfe_fwd(const float* voxels, const float* num_pts, int m, int p, int c,
                      float* out, void* stream);
int toda_mean_vfe_bwd(const float* grad_out, const float* num_pts, int m, int p, int c,
                      float* grad_voxels, void* stream);

/* ------------------------------------------------------------------------
 * Dynamic voxelisation (DynPillarVFE / DynMeanVFE): every in-range point is
 * kept, no caps.  points [n, width] is the collated batch (batch index in
 * column 0, x y z in columns 1-3); pillar != 0: key (b, x, y), x and y
 * tested (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:101-109);
 * 0: key (b, x, y, z), all axes tested (dynamic_mean_vfe.py:55-64).  A row
 * whose batch index is outside [0, batch) or NaN is dropped like an
 * out-of-range point.  Integer atomics only; every result is bit-reproducible.
 * ---------------------------------------------------------------------- */
size_t toda_dynvox_workspace_bytes(int n, int batch, const int32_t* grid_host, int pillar);
/* Pass 1: counts_dev[0] = M (distinct keys), counts_dev[1] = K (kept points).
 * The workspace carries the bitmap and keep positions on to toda_dynvox_index. */
int toda_dynvox_count(const float* points, int n, int width, int batch, const float* range_host, const float* vsize_host,
                      const int32_t* grid_host, int pillar, int32_t* counts_dev, void* ws, size_t ws_bytes, void* stream);
/* Pass 2, with the M and K of pass 1 (same arguments and workspace).  Replaces the mask + merge key +
 * torch.unique(return_inverse, return_counts) of dynamic_pillar_vfe.py:101-113 / dynamic_mean_vfe.py:55-66 and the
 * coordinate split of dynamic_pillar_vfe.py:141-148 / dynamic_mean_vfe.py:68-73:
 * keep [n] (uint8), rows [K] = original index of each kept point (ascending: reference points[mask]), inv [K] = unq_inv
 * (rows are numbered in torch.unique's ascending key order), cnt [M] = unq_cnt, coords [M, 4] = (b, z, y, x),
 * seg_off [M + 1] + seg_pts [K]: the kept rows of voxel v are seg_pts[seg_off[v] .. seg_off[v + 1]), ascending. */
int toda_dynvox_index(const float* points, int n, int width, int batch, const float* range_host, const float* vsize_host,
                      const int32_t* grid_host, int pillar, int m, int k, uint8_t* keep, int32_t* rows, int32_t* inv,
                      int32_t* seg_pts, int32_t* seg_off, int32_t* cnt, int32_t* coords, void* ws, size_t ws_bytes,
                      void* stream);
/* torch_scatter.scatter_mean / scatter_sum (dynamic_pillar_vfe.py:115, dynamic_mean_vfe.py:66, and the backward of
 * x_max[unq_inv]): out[v, c] = sum over the segment, in seg_pts order, of src[row, col0 + c]; row = rowmap[j] when rowmap
 * is given (points read in place through toda_dynvox_index's rows), else j.  divide != 0: / segment length. */
int toda_dynvox_seg_sum(const float* src, int ld, int col0, int ncol, const int32_t* rowmap, const int32_t* seg_off,
                        const int32_t* seg_pts, int m, int divide, float* out, void* stream);
/* dynamic_pillar_vfe.py:110-129: per kept row [points[:, 1:] (use_abs_xyz) or points[:, 4:], xyz - mean[inv],
 * xyz - pillar centre, (|xyz|)] written as the rows [K, f] the first Linear reads (no torch.cat).
 * offset_host = (x_offset, y_offset, z_offset) of dynamic_pillar_vfe.py:75-77; mean [M, 3] from toda_dynvox_seg_sum. */
int toda_dynvox_pillar_decorate(const float* points, int width, const int32_t* rows, const int32_t* inv,
                                const int32_t* coords, const float* mean, int k, const float* vsize_host,
                                const float* offset_host, int use_abs_xyz, int with_dist, float* out, int f, void* stream);
/* torch_scatter.scatter_max (dynamic_pillar_vfe.py:41): out [M, c] and arg [M, c] (row of the maximum; on a tie the
 * lowest row).  bwd: gx [k, c] = 0, gx[arg[v, c], c] = gout[v, c] (plain stores: a row belongs to one voxel). */
int toda_dynvox_seg_max_fwd(const float* x, int c, const int32_t* seg_off, const int32_t* seg_pts, int m, float* out,
                            int32_t* arg, void* stream);
int toda_dynvox_seg_max_bwd(const float* gout, const int32_t* arg, int m, int c, int k, float* gx, void* stream);
/* torch.cat([x, x_max[unq_inv, :]], dim=1) (dynamic_pillar_vfe.py:46): out [k, 2c]. */
int toda_dynvox_gather_concat(const float* x, const float* xmax, const int32_t* inv, int k, int c, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Grid index: a bitmap + popcount-rank dictionary over the (b, z, y, x)
 * lattice of one sparse level.  rank(coord) is the position of the site in
 * ascending ((b*D+z)*H+y)*W+x order, which is the canonical row order of
 * every index set this library generates.  Replaces spconv's hash table
 * (SparseConvTensor.indice_dict users, pcdet/models/backbones_3d/
 * spconv_backbone.py:77-117).
 * ---------------------------------------------------------------------- */
size_t toda_gridindex_bytes(int batch, const int32_t* shape_host /*[3] D H W*/);
/* Build the index of an existing coordinate list (any row order).
 * rowof[rank] = row.  Coordinates must be unique and in range. */
int toda_gridindex_from_coords(const int32_t* idx, int n, const int32_t* n_dev,
                               int batch, const int32_t* shape_host,
                               void* gi, int32_t* rowof, void* stream);
/* The same index for the VOXEL level, in O(sites): rank(coord) is NOT canonical here (ranks are handed out per
 * occupied 32-cell word by the site that set the word's lowest bit), which is all a level whose rows are in
 * caller order needs - rowof[rank] = row, toda_rulebook_subm / toda_rulebook_conv read it as before.  No sweep over
 * the lattice: the bitmap must be all zero on entry (gi_clean != 0: the caller guarantees it, e.g. through
 * toda_gridindex_clear after the previous use; 0: the call clears all of it first).  The coordinates of one list must
 * be unique: two rows with the same coordinate would race for one rowof entry (spconv never produces such a list). */
int toda_gridindex_from_coords_unordered(const int32_t* idx, int n, const int32_t* n_dev,
                                         int batch, const int32_t* shape_host,
                                         void* gi, int32_t* rowof, int gi_clean, void* stream);
/* Put the bitmap words of the listed sites back to zero (O(sites) instead of a memset of the lattice). */
int toda_gridindex_clear(const int32_t* idx, int n, const int32_t* n_dev, int batch,
                         const int32_t* shape_host, void* gi, void* stream);
/* Build the index of the OUTPUT set of a strided sparse convolution
 * (spconv.SparseConv3d, spconv_backbone.py:14-15,113-114) and emit its
 * coordinates in canonical order.  idx_out has room for out_cap rows. */
int toda_gridindex_from_conv(const int32_t* idx_in, int n_in, const int32_t* n_in_dev,
                             int batch, const int32_t* shape_in_host,
                             const int32_t* ksize_host, const int32_t* stride_host,
                             const int32_t* pad_host, const int32_t* shape_out_host,
                             void* gi_out, int32_t* idx_out, int32_t* n_out_dev,
                             int out_cap, void* stream);
/* The same from the INPUT level's grid index instead of its coordinate list: output stationary (one thread per
 * 32-cell output word ORs the input rows that reach it), no atomics, no clearing of gi_out, two launches; the input
 * row count never enters, so the levels of a backbone chain without a host round trip.  in_rows_marked != 0: gi_in was
 * built by toda_gridindex_from_coords_unordered, which also keeps one byte per lattice row (b, z, y) - input rows without
 * a site are then skipped after one byte load (the voxel level: most of its 123 k rows). */
int toda_gridindex_from_bitmap(const void* gi_in, int batch, const int32_t* shape_in_host,
                               const int32_t* ksize_host, const int32_t* stride_host,
                               const int32_t* pad_host, const int32_t* shape_out_host,
                               void* gi_out, int32_t* idx_out, int32_t* n_out_dev,
                               int out_cap, int in_rows_marked, void* stream);

/* Rulebook of spconv.SubMConv3d (spconv_backbone.py:12,78): out sites = in
 * sites.  nbr[k*n + o] = input row at o + (k - centre) * dilation or -1.
 * rowof may be NULL when rows are already in canonical order.
 * pair_cnt[K] (device) receives the number of valid pairs per offset (cnt_zeroed != 0: the caller has zeroed it,
 * e.g. every table's counters of a plan with one memset). */
int toda_rulebook_subm(const int32_t* idx, int n, int batch, const int32_t* shape_host,
                       const int32_t* ksize_host, const int32_t* dilation_host,
                       const void* gi, const int32_t* rowof,
                       int32_t* nbr, int32_t* pair_cnt, int cnt_zeroed, void* stream);
/* Rulebook of spconv.SparseConv3d: nbr_o2i[k*n_out + o] = input row feeding
 * output o through offset k; nbr_i2o[k*n_in + i] = output row fed by input i
 * through offset k (used by dgrad).  idx_out / gi_in / rowof_in (optional, NULL = unknown): the output coordinates
 * and the INPUT level's grid index (+ its rowof when the input rows are not canonical); with them the o2i table is
 * written output-stationary (complete coalesced rows) instead of a 0xFF fill + scattered stores. */
int toda_rulebook_conv(const int32_t* idx_in, int n_in, int batch,
                       const int32_t* shape_in_host, const int32_t* ksize_host,
                       const int32_t* stride_host, const int32_t* pad_host,
                       const int32_t* shape_out_host, const void* gi_out, int n_out,
                       int32_t* nbr_o2i, int32_t* nbr_i2o, int32_t* pair_cnt,
                       const int32_t* idx_out, const void* gi_in, const int32_t* rowof_in,
                       int cnt_zeroed, void* stream);

/* ------------------------------------------------------------------------
 * Sparse convolution arithmetic (spconv SubMConv3d / SparseConv3d forward and
 * the autograd backward reached from tools/train_utils/train_utils.py:55).
 * All three are gather -> fp32 MFMA GEMM -> store, output stationary, no
 * atomics in fwd/dgrad.
 * ---------------------------------------------------------------------- */
/* Re-order weights [Cout][K][Cin] into the MFMA fragment order the kernels
 * read.  transpose=0: operand for fwd (gathers Cin, produces Cout).
 * transpose=1: operand for dgrad (gathers Cout, produces Cin); flip_k=1
 * additionally reverses the offset order (SubM dgrad reuses the forward
 * table through the point symmetry of the stencil). */
size_t toda_spconv_packed_weight_floats(int k_vol, int c_gather, int c_produce);
/* Matrix path of the gather-GEMMs (forward and data gradient of spconv SubMConv3d / SparseConv3d, reference
 * pcdet/models/backbones_3d/spconv_backbone.py:77-125,191-240), process-wide: 0 = native - fp32 operands on
 * v_mfma_f32_16x16x4_f32; 1 = split - every fp32 operand taken apart EXACTLY into three bf16 values (hi + mid + lo = x),
 * six of the nine cross products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (the three dropped ones are below
 * 2^-22 of the product each, 2^-25 on average: the size of an fp32 product's own rounding), 6/16 of the matrix cycles, for the channel pairs toda_spconv_split_supported names; every other
 * pair runs native under either path.  Initial value: environment TODA_MM = native | split (default split: it holds the
 * gates of tests/test_gpu_split.py - oracle parity at the unchanged tolerance, error against fp64 <= 1.5 x native, bit-reproducible).  The packed operand of a
 * supported pair is written in the format of the path current at PACK time (toda_spconv_packed_weight_floats covers both)
 * and must be multiplied under the same path: set the path before packing, re-pack after changing it.  The same switch selects the
 * arithmetic of toda_spconv_wgrad (32 / 64-channel pairs and 128 x 128) and of toda_conv3x3s2_* / toda_deconv_* (operands split when
 * they are staged; no packed operand involved; TODA_PG_SPLIT=0 keeps those on the fp32 instructions). */
int toda_matrix_path(void);
int toda_set_matrix_path(int mode);
int toda_spconv_split_supported(int c_gather, int c_produce);
int toda_spconv_pack_weight(const float* w, int cout, int k_vol, int cin,
                            int transpose, int flip_k, float* wp, void* stream);
/* The same for n weights in one launch (the forward and the data-gradient operand of every sparse convolution of a
 * backbone, once per optimizer step).  All array arguments are HOST arrays of length n; wp_host[i] receives
 * toda_spconv_packed_weight_floats(k_vol[i], c_gather, c_produce) floats. */
int toda_spconv_pack_weights(int n, const float* const* w_host, const int32_t* cout_host, const int32_t* k_vol_host,
                             const int32_t* cin_host, const int32_t* transpose_host, const int32_t* flip_k_host,
                             float* const* wp_host, void* stream);
/* out[o, :] = bias + sum_k Wp[k] . in[nbr[k*n_out + o], :]   (rows with nbr<0 skipped).
 * `in` has n_in rows of c_gather floats (the table is read through a bounds-checked buffer
 * descriptor, so n_in * c_gather * 4 must be < 4 GiB). */
int toda_spconv_gather_gemm(const float* in, int n_in, int c_gather, const float* wp,
                            const int32_t* nbr, int n_out, int k_vol, int c_produce,
                            const float* bias /*nullable*/, float* out, void* stream);
/* Same, visiting the output rows in the order `order[n_out]` (a permutation, nullable = canonical): results are
 * identical, only the assignment of rows to waves changes (the class-sorted data gradient below is built on it). */
int toda_spconv_gather_gemm_ordered(const float* in, int n_in, int c_gather, const float* wp,
                                    const int32_t* nbr, int n_out, int k_vol, int c_produce,
                                    const float* bias, float* out, const int32_t* order, void* stream);

/* Data gradient of a STRIDED SparseConv3d (autograd backward of spconv_backbone.py:118-160's spconv2/3/4 and conv_out):
 * an input site reaches an output only through the kernel offsets congruent to (coordinate + padding) modulo the
 * stride on every axis, i.e. 1..8 of the 27 offsets, all of them populated.  toda_rulebook_class_order regroups the
 * rows (= the conv's INPUT sites, in_coords [n_in][4] = b,z,y,x) by residue class inside 8192-row blocks:
 * order[pos] = row, cls_sorted[pos] = class.  toda_spconv_gather_gemm_classed is toda_spconv_gather_gemm_ordered whose
 * waves walk only the candidate offsets of their class (ksize / stride / padding: HOST int[3], z,y,x).  Results are
 * bit-identical to the plain call. */
int toda_rulebook_class_order(const int32_t* in_coords, int n_in, const int32_t* stride_host, const int32_t* padding_host,
                              int32_t* order, unsigned char* cls_sorted, void* stream);
int toda_spconv_gather_gemm_classed(const float* in, int n_in, int c_gather, const float* wp, const int32_t* nbr, int n_out,
                                    int k_vol, int c_produce, const float* bias, float* out, const int32_t* order,
                                    const unsigned char* cls_sorted, const int32_t* ksize_host, const int32_t* stride_host,
                                    const int32_t* padding_host, void* stream);
/* The same contraction for the narrow K = 27 layers (<= 32 gathered, <= 32 produced channels: conv_input, the 16-channel SubM
 * level, the strided 16 -> 32 and their data gradients - reference pcdet/models/backbones_3d/spconv_backbone.py:92-115): per
 * offset a wave compacts the rows that have a neighbour, so only real pairs are gathered and multiplied.  w is the PLAIN weight
 * [w_cout][27][w_cin]; transpose / flip_k as in toda_spconv_pack_weight (data gradient: transpose = 1, flip_k = 1 for SubM). */
int toda_spconv_gather_gemm_compact_supported(int c_gather, int c_produce, int k_vol);
int toda_spconv_gather_gemm_compact(const float* in, int n_in, int c_gather, const float* w, int w_cout, int w_cin,
                                    int transpose, int flip_k, const int32_t* nbr, int n_out, int k_vol, int c_produce,
                                    const float* bias /*nullable*/, float* out, void* stream);
/* The same launch with the following BatchNorm1d's moments from the epilogue (the <= 16-channel layers of the backbone,
 * reference spconv_backbone.py:21-25): sums = 2 c results + [2 c][workgroups] scratch as toda_spconv_gather_gemm_stats;
 * blocks_out == NULL: folded by the call, else left for toda_bn_finalize_partials with *blocks_out (host) partials per column. */
size_t toda_spconv_gather_gemm_compact_stats_doubles(int n_out, int c_produce);
int toda_spconv_gather_gemm_compact_stats(const float* in, int n_in, int c_gather, const float* w, int w_cout, int w_cin,
                                          int transpose, int flip_k, const int32_t* nbr, int n_out, int k_vol,
                                          int c_produce, const float* bias /*nullable*/, float* out, double* sums,
                                          size_t sums_doubles, int* blocks_out /*nullable*/, void* stream);

/* dw[co][k][ci] = sum_o in[nbr[k*n_out+o], ci] * dout[o, co] */
size_t toda_spconv_wgrad_workspace_bytes(int n_out, int k_vol, int cin, int cout);
int toda_spconv_wgrad(const float* in, int n_in, const float* dout, const int32_t* nbr,
                      int n_out, int k_vol, int cin, int cout, float* dw,
                      void* ws, size_t ws_bytes, void* stream);
/* SparseConvTensor.dense() as used by HeightCompression
 * (pcdet/models/backbones_2d/map_to_bev/height_compression.py:21-23):
 * dense[b, c, z, y, x] = feat[row, c]; the caller views it as [B, C*D, H, W].
 * fwd zero-fills `dense` itself. */
int toda_sparse_to_dense_fwd(const float* feat, const int32_t* idx, int n, int c,
                             int batch, const int32_t* shape_host, float* dense, void* stream);
int toda_sparse_to_dense_bwd(const float* grad_dense, const int32_t* idx, int n, int c,
                             int batch, const int32_t* shape_host, float* grad_feat, void* stream);

/* PointPillarScatter (pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:14-37):
 * canvas[b, c, y, x] = pillar[row, c] for coords (b, z=0, y, x). */
int toda_pillar_scatter_fwd(const float* feat, const int32_t* idx, int n, int c,
                            int batch, int ny, int nx, float* canvas, void* stream);
int toda_pillar_scatter_bwd(const float* grad_canvas, const int32_t* idx, int n, int c,
                            int batch, int ny, int nx, float* grad_feat, void* stream);

/* ------------------------------------------------------------------------
 * Fused per-channel statistics / normalise+ReLU over the active rows of a
 * sparse level: the nn.BatchNorm1d(eps=1e-3, momentum=0.01) + nn.ReLU pair of
 * post_act_block (spconv_backbone.py:8-27).
 * ---------------------------------------------------------------------- */
/* sums[0:c] = sum_rows x, sums[c:2c] = sum_rows x*x  (fp32 inside a thread, fp64 across threads and blocks, fixed
 * order: bit-reproducible).  `sums` must hold toda_rows_reduce_doubles(n, c) doubles: the first 2c are the result,
 * the rest is per-block scratch (also for toda_rows_bn_bwd). */
size_t toda_rows_reduce_doubles(int n, int c);
int toda_rows_moments(const float* x, int n, int c, double* sums /*[toda_rows_reduce_doubles(n, c)]*/,
                      void* stream);
/* y = relu?(x * scale[c] + shift[c] (+ residual)) */
int toda_rows_affine_act(const float* x, const float* scale, const float* shift,
                         const float* residual /*nullable*/, int n, int c, int relu,
                         float* y, void* stream);

/* Batch statistics -> per-channel mean / invstd / scale / shift, plus nn.BatchNorm1d's
 * running-statistic update (momentum, unbiased running_var; the biased value for n == 1).  training == 0: running stats.
 * Training mode with n < 1 is an argument error, as in toda_bn_finalize_partials. */
int toda_bn_finalize(const double* sums /*[2c] from toda_rows_moments*/, int n, int c,
                     const float* gamma, const float* beta, float* running_mean /*nullable*/,
                     float* running_var /*nullable*/, float momentum, float eps, int training,
                     float* mean, float* invstd, float* scale, float* shift, void* stream);
/* The same with the fold of the per-workgroup partial sums inside (training mode): toda_spconv_gather_gemm_stats_partials leaves
 * `blocks` partials per column behind the 2c result slots of `sums`; one launch folds them in the fixed order of the separate
 * fold, writes the totals to sums[0:2c] and finalises.  Saves one launch per BatchNorm1d of the sparse backbone. */
int toda_bn_finalize_partials(double* sums, int blocks, int n, int c, const float* gamma, const float* beta,
                              float* running_mean /*nullable*/, float* running_var /*nullable*/, float momentum, float eps,
                              float* mean, float* invstd, float* scale, float* shift, void* stream);
/* Backward of the same pair.  stats = [mean | invstd | scale | shift] (4*c floats, as written by
 * toda_bn_finalize into one buffer).  dz = dy * (x*scale+shift > 0) (relu != 0) or dy;
 * sums[0:c] = sum dz = d(beta), sums[c:2c] = sum dz*xhat = d(gamma) (zeroed and filled by the call); the same 2c values rounded
 * to float32 follow at ((float*)(sums + 2c))[0:2c] (what an optimizer wants: no conversion pass);
 * dx = gamma * invstd * (dz - sums[0:c]/n - xhat * sums[c:2c]/n), xhat = (x - mean) * invstd. */
int toda_rows_bn_bwd(const float* dy, const float* x, const float* stats, const float* gamma,
                     int n, int c, int relu, double* sums /*[toda_rows_reduce_doubles(n, c)]*/, float* dx,
                     void* stream);

/* The same with a shortcut branch (SparseBasicBlock, spconv_backbone.py:30-66: y = relu(bn2(x) + identity)): the ReLU
 * mask is recomputed from x*scale+shift + residual, dres (nullable) receives dz = the gradient of the shortcut. */
int toda_rows_bn_bwd_res(const float* dy, const float* x, const float* residual /*nullable*/, const float* stats,
                         const float* gamma, int n, int c, int relu, double* sums, float* dx,
                         float* dres /*nullable*/, void* stream);
/* ... and with the column sums of dx, dx_colsum[0:c] = sum over rows of dx: the bias gradient of the convolution that produced
 * x (SparseBasicBlock's convolutions have a bias, spconv_backbone.py:37-40; autograd's `grad_output.sum(0)` pass over dx
 * disappears).  Taken while dx is written; fixed-order fold (deterministic).  colsum_ws: toda_rows_bn_bwd_colsum_doubles(n, c)
 * doubles; both pointers NULL: exactly toda_rows_bn_bwd_res. */
size_t toda_rows_bn_bwd_colsum_doubles(int n, int c);
int toda_rows_bn_bwd_res_colsum(const float* dy, const float* x, const float* residual /*nullable*/, const float* stats,
                                const float* gamma, int n, int c, int relu, double* sums, float* dx,
                                float* dres /*nullable*/, double* colsum_ws /*nullable*/, float* dx_colsum /*nullable*/,
                                void* stream);

/* Single-pass training-mode nn.BatchNorm2d (+ nn.ReLU) of the BEV neck and heads (base_bev_backbone.py:37-58,
 * center_head.py:20-28, 73-80; replaces torch's batch_norm + relu_ pair and their backward): the values of a channel sit in
 * registers between the statistics and the normalisation, so forward reads x once and writes y once and backward reads x
 * and dy once and writes dx once.  Two forms: one workgroup per channel (batch 1 / 2: hw <= 36864, batch 4: hw <= 16384;
 * backward then reads x a second time), or - batch 2 / 4 with a `sync` workspace, hw <= 36864 - one workgroup per (channel,
 * sample) plane, the workgroups of a channel exchanging two fp64 partial results through `sync`; the library takes the
 * per-plane form where the per-channel one does not fit or measured slower (large backward planes).  hw % 4 == 0 uses 16-byte
 * accesses, any other hw dword accesses.
 * sync: toda_bn2d_sync_bytes() bytes, zeroed ONCE by the caller, used by one stream at a time, channels <= 4096; epoch:
 * a non-zero number the caller does not repeat on that workspace (increment per call) - nothing is reset between launches.
 * save = [2][c] floats (mean, 1/sqrt(var + eps)) from forward for backward.  running_mean / running_var (nullable
 * together) are updated in place like nn.BatchNorm2d does (momentum, unbiased variance).  relu != 0: y = max(bn(x), 0);
 * backward recomputes the mask from x with the forward's expression.  Deterministic (fixed summation order). */
int toda_bn2d_supported(int batch, int c, int hw);
size_t toda_bn2d_sync_bytes(void);
int toda_bn2d_fwd(const float* x, int batch, int c, int hw, const float* gamma, const float* beta,
                  float* running_mean /*nullable*/, float* running_var /*nullable*/, float momentum, float eps, int relu,
                  float* y, float* save, void* sync /*nullable*/, unsigned epoch, void* stream);
int toda_bn2d_bwd(const float* x, const float* dy, int batch, int c, int hw, const float* gamma, const float* beta,
                  const float* save, int relu, float* dx, float* dgamma, float* dbeta, void* sync /*nullable*/,
                  unsigned epoch, void* stream);
/* The same pair with y / dy a CHANNEL SLICE [channel0, channel0 + c) of a wider [batch][channels][hw] tensor: the up-sampling
 * deblocks of the BEV neck write straight into the concatenated map and read its gradient in place, so torch.cat and the copies
 * of its backward (reference pcdet/models/backbones_2d/base_bev_backbone.py:104-107) never run. */
int toda_bn2d_fwd_into(const float* x, int batch, int c, int hw, const float* gamma, const float* beta,
                       float* running_mean /*nullable*/, float* running_var /*nullable*/, float momentum, float eps, int relu,
                       float* y, int y_channels, int y_channel0, float* save, void* sync /*nullable*/, unsigned epoch,
                       void* stream);
int toda_bn2d_bwd_from(const float* x, const float* dy, int dy_channels, int dy_channel0, int batch, int c, int hw,
                       const float* gamma, const float* beta, const float* save, int relu, float* dx, float* dgamma,
                       float* dbeta, void* sync /*nullable*/, unsigned epoch, void* stream);

/* ------------------------------------------------------------------------
 * CenterHead target assignment (pcdet/models/dense_heads/center_head.py:103-219,
 * pcdet/models/model_utils/centernet_utils.py:9-69): gaussian heat-maps,
 * regression targets, flat indices and masks for one head group.
 * gt_boxes [B, G, 8] = (x y z dx dy dz heading cls_in_head(1-based, 0 = pad)).
 * ---------------------------------------------------------------------- */
int toda_center_assign(const float* gt_boxes, int batch, int n_gt, int code_size,
                       int num_classes, int fm_w, int fm_h,
                       const float* range_host /*[6]*/, const float* vsize_host /*[3]*/,
                       int fm_stride, int max_objs, double gaussian_overlap, int min_radius,
                       float* heatmap /*[B, num_classes, fm_h, fm_w], zero-filled by the call*/,
                       float* ret_boxes /*[B, max_objs, code_size]*/,
                       int64_t* inds /*[B, max_objs]*/, int64_t* mask /*[B, max_objs]*/,
                       void* stream);

/* ------------------------------------------------------------------------
 * Anchor target assignment (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 with
 * POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False, MATCH_HEIGHT False) for the whole batch and every anchor class: two launches,
 * nothing read back.  anchors_host: n_classes device pointers to the class tables [locs = nz*ny*nx, per_loc = sizes*rotations,
 * anchor_stride >= 7]; gt_boxes [B, M, gt_stride >= 8], class id (1-based, 0 = padding) in the last column; slot_of [n_ids]
 * (device) maps a class id to its anchor class, -1 for none.  Nearest-axis BEV IoU in fp32 with the operation order of
 * box_utils.boxes3d_nearest_bev_iou; per anchor the best gt (lowest index on a tie), per gt the maximum over the anchors;
 * positive: best >= matched or IoU == a gt's non-zero maximum; background (0): best < unmatched; otherwise -1.
 * targets = ResidualCoder.encode_torch of the best gt for positives (code_size = 6 + (sincos ? 2 : 1) + extra columns
 * shared by anchors and gts), zero elsewhere; weights = 1 on positives.  multihead_order 0: rows in (z, y, x, class, size,
 * rot) order, 1: class-major then (size, rot, z, y, x).  Integer atomics only: bit-reproducible.
 * ws: toda_anchor_assign_workspace_bytes(batch, n_gt) bytes.
 * ---------------------------------------------------------------------- */
size_t toda_anchor_assign_workspace_bytes(int batch, int n_gt);
int toda_anchor_assign(const void* const* anchors_host, const int32_t* locs_host, const int32_t* per_loc_host,
                       const float* matched_host, const float* unmatched_host, int n_classes, int anchor_stride,
                       const float* gt_boxes, int batch, int n_gt, int gt_stride, const int32_t* slot_of, int n_ids,
                       int code_size, int encode_angle_by_sincos, int multihead_order,
                       int32_t* labels /*[B, A]*/, float* targets /*[B, A, code_size]*/, float* weights /*[B, A]*/,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Rotated BEV IoU and greedy NMS (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-326 and the host
 * sweep of iou3d_nms.cpp:100-135, reached through model_nms_utils.class_agnostic_nms from
 * CenterHead.generate_predicted_boxes, center_head.py:291-300).  Boxes are rows of 7 floats
 * (x, y, z, dx, dy, dz, heading).  toda_nms_rotated expects the boxes sorted by descending score
 * and leaves the kept indices (ascending = score order) and their count on the device.
 * ---------------------------------------------------------------------- */
int toda_boxes_iou_bev(const float* boxes_a, int na, const float* boxes_b, int nb,
                       float* iou /*[na, nb]*/, void* stream);
/* Intersection AREA of the rotated BEV rectangles (iou3d_nms_kernel.cu boxes_overlap_kernel, used by
 * iou3d_nms_utils.boxes_iou3d_gpu :52-82 for the recall record of detector3d_template.py:287-328). */
int toda_boxes_overlap_bev(const float* boxes_a, int na, const float* boxes_b, int nb,
                           float* overlap /*[na, nb]*/, void* stream);
size_t toda_nms_workspace_bytes(int n);
int toda_nms_rotated(const float* boxes_sorted, int n, float thresh, int64_t* keep /*[n]*/,
                     int32_t* n_keep_dev, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * SECONDHead (pcdet/models/roi_heads/second_head.py, proposal_target_layer.py).
 * toda_roi_grid_pool_bev: the rotated-RoI grid pool of second_head.py:53-110 in one launch for the batch - for roi r of sample
 * r / N, F.affine_grid (align_corners=False) of its 2 x 3 matrix, then F.grid_sample (bilinear, zero padding) of the map.
 * feat [B, C, H, W] fp32 NCHW; rois [B, N, roi_stride >= 7] (x, y, z, dx, dy, dz, heading, ...); step_x / step_y = voxel size x
 * DOWNSAMPLE_RATIO; out [B * N, C, G, G] fp32, fully written.  Forward only (the reference detaches both inputs); no atomics.
 * toda_roi_iou3d_max: per roi, the best 3-D IoU against the valid gts of its sample and the index of that gt
 * (proposal_target_layer.py:92-96 + get_max_iou_with_same_class :194-228).  gt [B, M, gt_stride >= 8], label in the last
 * column; valid gts = last row with a non-zero sum + 1, at least one.  by_class: only gts whose (long) label equals the roi's
 * label (roi_labels [B, N] int64, may be NULL otherwise).  No eligible gt: IoU 0, index 0; ties: the lowest gt index.
 * ---------------------------------------------------------------------- */
int toda_roi_grid_pool_bev(const float* feat, int B, int C, int H, int W, const float* rois, int N, int roi_stride,
                           float min_x, float min_y, float step_x, float step_y, int grid_size, float* out, void* stream);
int toda_roi_iou3d_max(const float* rois, int B, int N, int roi_stride, const int64_t* roi_labels, const float* gt, int M,
                       int gt_stride, int by_class, float* max_iou /*[B, N]*/, int64_t* argmax /*[B, N]*/, void* stream);

/* ------------------------------------------------------------------------
 * VoxelRCNNHead (pcdet/models/roi_heads/voxelrcnn_head.py, ops/pointnet2/pointnet2_stack/voxel_{query_utils,pool_modules}.py).
 * toda_voxel_query: voxel_query_gpu.cu's scan (dz, dy, dx over [-range, range], keep dist2 <= radius^2 in scan order, the
 * first hit fills the row, stop at nsample hits) over one level.  new_xyz [M, 3] fp32, new_coords [M, 4] int32 (b, z, y, x);
 * xyz [N, 3] voxel centres of the level's rows; gi = the level's grid-index buffer (toda_gridindex_*), rowof its rank -> row
 * map or NULL when the ranks are the rows; shape_host = (Z, Y, X), ranges_host = (z, y, x).  idx [M, nsample] int32 = rows of
 * the level (all zero for an empty ball), empty [M] uint8.  Grid points with b outside [0, batch) get empty balls.
 * toda_voxel_pool_moments: mean (3) and biased covariance (3 x 3) of d = xyz[idx] - new_xyz (0 for empty balls) over all
 * M x nsample entries, fp64, fixed-order; ws [toda_voxel_pool_moments_doubles()] doubles, the result in ws[0:12].
 * toda_voxel_pool_fwd: out[m, c] = max_s relu(f[idx[m, s], c] [not empty] + ab[c, 0:3] . d_ms + ab[c, 3]); f [N, C], ab [C, 4],
 * out [M, C]; arg [M, C] uint8 (NULL: not stored) = first arg-max s, 0xff where out is 0.
 * toda_voxel_pool_table: the inverse neighbour table of any idx [M, nsample] over N rows (the name is kept for ABI stability):
 * off [N + 1] (exclusive prefix of the per-row counts), ent [M x nsample] = entries m * nsample + s of row n at
 * ent[off[n] .. off[n + 1]), ascending; empty balls are left out; any nsample with M x nsample < 2^31.  Three consumers:
 * toda_voxel_pool_bwd_feat, toda_sa_gather_bwd_feat and toda_bev_interp_bwd (the last two below).
 * toda_voxel_pool_bwd_feat: gf [N, C] = d out / d f through the table; toda_voxel_pool_bwd_pos: gab [C, 4] = d out / d ab,
 * ws [toda_voxel_pool_bwd_pos_doubles(C)] doubles.  Integer atomics only: every result is bit-reproducible.
 * ---------------------------------------------------------------------- */
int toda_voxel_query(const float* new_xyz, const int32_t* new_coords, int M, const float* xyz, int N, const void* gi, const int32_t* rowof,
                     int batch, const int32_t* shape_host, float radius, const int32_t* ranges_host, int nsample, int32_t* idx,
                     uint8_t* empty, void* stream);
size_t toda_voxel_pool_moments_doubles(void);
int toda_voxel_pool_moments(const int32_t* idx, const uint8_t* empty, int M, int nsample, const float* xyz, int N, const float* new_xyz,
                            double* ws, void* stream);
int toda_voxel_pool_fwd(const float* f, int N, int C, const int32_t* idx, const uint8_t* empty, int M, int nsample, const float* xyz,
                        const float* new_xyz, const float* ab, float* out, uint8_t* arg, void* stream);
size_t toda_voxel_pool_table_bytes(int M, int nsample, int N);
int toda_voxel_pool_table(const int32_t* idx, const uint8_t* empty, int M, int nsample, int N, int32_t* off, int32_t* ent, void* ws,
                          size_t ws_bytes, void* stream);
int toda_voxel_pool_bwd_feat(const float* gout, const uint8_t* arg, int M, int nsample, int C, const int32_t* off, const int32_t* ent,
                             int N, float* gf, void* stream);
size_t toda_voxel_pool_bwd_pos_doubles(int C);
int toda_voxel_pool_bwd_pos(const float* gout, const uint8_t* arg, const int32_t* idx, const uint8_t* empty, int M, int nsample, int C,
                            const float* xyz, int N, const float* new_xyz, double* ws, float* gab, void* stream);

/* ------------------------------------------------------------------------
 * PV-RCNN's PointNet++ stack layer (pcdet/ops/pointnet2/pointnet2_stack, backbones_3d/pfe/voxel_set_abstraction.py).
 * toda_fps: farthest point sampling of every sample of a stacked cloud xyz [N, 3]; starts_host [batch + 1] host offsets of the
 * samples; idx [batch, npoint] int32 sample-local indices, equal to sampling_gpu.cu's farthest_point_sampling_kernel (first index
 * 0, temp from 1e10, d = dx dx + dy dy + dz dz; ties to the smallest bit-reversed k mod opt_n_threads(n), the order its block
 * tree prefers, then the smallest k).  mode 1: one
 * workgroup per sample (temp [N] fp32 scratch); mode 2: co-resident workgroup groups meeting at a bounded inter-workgroup
 * barrier (ws [toda_fps_workspace_bytes]; TODA_FAULT_FPS if a wait gives up); mode 0 picks by sample size and falls back to
 * mode 1 when the groups do not fit toda_fps_resident_blocks().
 * toda_ball_query_stack: for every query new_xyz [M, 3] (sample by new_start [batch + 1], device), the points of its sample
 * (xyz_start [batch + 1], device) in ascending index with d2 < r^2, for nr nested radii in one scan: idx_host[r] [M, nsample_r]
 * int32 rows of xyz (the first hit fills the row, stop at nsample_r hits; zeros for an empty ball), empty_host[r] [M] uint8.
 * toda_sa_gather_fwd: layer 1 of a StackSAModuleMSG MLP after its feature GEMM: z [M x nsample, C] = P[idx] + wd [C, 3] . d,
 * d = xyz[idx] - new_xyz, 0 for an empty ball.  Backward: gP [N, C] through the inverse neighbour table of
 * toda_voxel_pool_table (toda_sa_gather_bwd_feat), gwd [C, 3] from fp64 partials (ws [toda_sa_gather_bwd_pos_doubles(C)]).
 * toda_sa_max_fwd: out [M, C] = max over nsample (<= 254) of y [M x nsample, C], arg [M, C] uint8 the first arg-max, whatever
 * the sign of the maximum (F.max_pool2d's gradient); toda_sa_max_bwd: gy [M x nsample, C].
 * toda_bev_interp_fwd: voxel_set_abstraction.py's bilinear_interpolate_torch from map [B, C, H, W] at xy [K, 2] (column, row)
 * of sample bidx [K]: out [K, C]; taps [K, 4] pixel ids (b H + y) W + x of Ia Ib Ic Id and wts [K, 4] their weights (both NULL:
 * not stored).  toda_bev_interp_bwd: gmap [B, C, H, W] through the pixel table of taps (toda_voxel_pool_table with
 * M = K, nsample = 4, N = B H W).  No float atomics: every result is bit-reproducible.
 * ---------------------------------------------------------------------- */
int toda_fps_resident_blocks(void);
size_t toda_fps_workspace_bytes(int batch, int npoint);
int toda_fps(const float* xyz, const int32_t* starts_host, int batch, int npoint, int mode, float* temp, int32_t* idx, void* ws,
             size_t ws_bytes, void* stream);
int toda_ball_query_stack(const float* xyz, int N, const int32_t* xyz_start, const float* new_xyz, const int32_t* new_start, int batch,
                          int M, int nr, const float* radii_host, const int32_t* nsample_host, int32_t* const* idx_host,
                          uint8_t* const* empty_host, void* stream);
int toda_sa_gather_fwd(const float* P, int N, int C, const float* wd, const int32_t* idx, const uint8_t* empty, int M, int nsample,
                       const float* xyz, const float* new_xyz, float* z, void* stream);
int toda_sa_gather_bwd_feat(const float* gz, int M, int nsample, int C, const int32_t* off, const int32_t* ent, int N, float* gP,
                            void* stream);
size_t toda_sa_gather_bwd_pos_doubles(int C);
int toda_sa_gather_bwd_pos(const float* gz, const int32_t* idx, const uint8_t* empty, int M, int nsample, int C, const float* xyz, int N,
                           const float* new_xyz, double* ws, float* gwd, void* stream);
int toda_sa_max_fwd(const float* y, int M, int nsample, int C, float* out, uint8_t* arg, void* stream);
int toda_sa_max_bwd(const float* g, const uint8_t* arg, int M, int nsample, int C, float* gy, void* stream);
int toda_bev_interp_fwd(const float* map, int B, int C, int H, int W, const float* xy, const int32_t* bidx, int K, float* out,
                        int32_t* taps, float* wts, void* stream);
int toda_bev_interp_bwd(const float* g, int K, int C, const int32_t* off, const int32_t* ent, const float* wts, int B, int H, int W,
                        float* gmap, void* stream);

/* ------------------------------------------------------------------------
 * Point-table primitives of the TODA mixing processors and the data processor's range mask.
 * They replace, on the device, the numpy / single-thread C++ work the reference does per scene in
 * DataLoader workers:
 *   - roiaware_pool3d_utils.points_in_boxes_cpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168),
 *     box_utils.remove_points_in_boxes3d (pcdet/utils/box_utils.py:75-89), augmentor_utils.get_points_in_box
 *     (pcdet/datasets/augmentor/augmentor_utils.py:474-491)                       -> toda_points_in_boxes
 *   - the azimuth-sector test of PolarMix swap (inter_domain_point_polarmix.py:76-98) -> toda_points_sector
 *   - the crop test of CutMix (inter_domain_point_cutmix.py:44-54) and mask_points_by_range
 *     (pcdet/utils/common_utils.py:60-63)                                         -> toda_points_rect
 *   - the cylinder cells of LaserMix (inter_domain_point_lasermix.py:89-165)       -> toda_points_polar_cell
 *   - the elevation bands of spherical LaserMix (inter_domain_point_lasermix.py:40-47,62-80) -> toda_points_pitch_band
 *   - PolarMix's sector cut at a random range (swap_with_range, inter_domain_point_polarmix.py:101-123) and the
 *     elevation test of swap(use_pitch=True) (:81-93)                  -> toda_points_polar_select, toda_points_pitch_range
 *   - boolean-mask indexing / np.delete / np.concatenate of point arrays           -> toda_rows_select_append
 *   - rotate_copy's point rotation (inter_domain_point_polarmix.py:160-188)        -> toda_points_rotate_z
 * points: [n, c] fp32 rows (x, y, z, ...).  n_dev (nullable): device int32, rows = min(n, *n_dev), so
 * chains run without host syncs.  flags / cells are int32 per row.
 * ---------------------------------------------------------------------- */
/* flags[j] = 1 iff some box (rows of box_stride >= 7 floats: x y z dx dy dz heading) contains point j.
 * mode 0: roiaware test (margin 1e-2, strict), mode 1: get_points_in_box test (margin 1e-1, inclusive).
 * mode 2: points_in_boxes_gpu (roiaware_pool3d_kernel.cu:23-36, 313-336; margin 1e-5): flags[j] = index of the FIRST
 * box that holds point j, -1 for none (used to cut the ground-truth database out of the scenes). */
int toda_points_in_boxes(const float* points, int n, const int32_t* n_dev, int c, const float* boxes,
                         int k, int box_stride, int mode, int32_t* flags, void* stream);
/* flags[j] = lo < -atan2(y, x) < hi   (yaw as an fp32 value, compared in fp64) */
int toda_points_sector(const float* points, int n, const int32_t* n_dev, int c, double lo, double hi,
                       int32_t* flags, void* stream);
/* closed == 0: lo < (x, y) < hi;  closed == 1: lo <= (x, y) <= hi */
int toda_points_rect(const float* points, int n, const int32_t* n_dev, int c, const double* lo_xy_host,
                     const double* hi_xy_host, int closed, int32_t* flags, void* stream);
/* cell[j] = i * n_dis + j' for yaw' in (yaw_edges[i], yaw_edges[i+1]] and range in (dis_edges[j'], dis_edges[j'+1]],
 * yaw' = wrap(-atan2(y, x) + phase), range = clip(sqrt(x^2 + y^2), dis_lo, dis_hi); -1 when outside every cell */
int toda_points_polar_cell(const float* points, int n, const int32_t* n_dev, int c, float phase,
                           const double* yaw_edges_host, int n_yaw, const double* dis_edges_host, int n_dis,
                           float dis_lo, float dis_hi, int32_t* cell, void* stream);
/* flags[j] = [yaw_mode 1: lo < yaw < hi | 2: yaw < lo or yaw > hi]  and  [dis_mode 0: - | 1: range < dis_th | 2: range > dis_th]
 * and, with pitch_range_dev != NULL, [range > 1 and -atan2(z, range) outside [pitch_range_dev[0], pitch_range_dev[1]]];
 * yaw = -atan2(y, x) and range = sqrt(x^2 + y^2) as fp32 values, thresholds compared in fp64 (round them to fp32 where numpy would). */
int toda_points_polar_select(const float* points, int n, const int32_t* n_dev, int c, double lo, double hi, int yaw_mode,
                             int dis_mode, double dis_th, const float* pitch_range_dev, int32_t* flags, void* stream);
/* range_dev[0:2] = min, max of -atan2(z, range) over the rows with range > 1 (+inf, -inf when there is none); deterministic. */
size_t toda_points_pitch_range_workspace_bytes(void);
int toda_points_pitch_range(const float* points, int n, const int32_t* n_dev, int c, float* range_dev, void* ws,
                            size_t ws_bytes, void* stream);
/* band[j] = i for edges[i + 1] < e <= edges[i] (n_bands + 1 descending edges, radians, host array), e = clip(atan2(z_offset + z,
 * range), clip_lo, clip_hi) in fp32; -1 when no band holds it */
int toda_points_pitch_band(const float* points, int n, const int32_t* n_dev, int c, float z_offset, float clip_lo,
                           float clip_hi, const double* edges_host, int n_bands, int32_t* band, void* stream);
/* Stable compaction: rows with (keys[j] == match) != invert (all rows when keys == NULL) are appended, in
 * order, at dst[*cursor_dev ...]; *cursor_dev += count.  Rows beyond cap_rows are dropped (the cursor still
 * counts them, so the caller sees the overflow). */
size_t toda_rows_select_workspace_bytes(int n);
int toda_rows_select_append(const float* src, int n, const int32_t* n_dev, int c, const int32_t* keys,
                            int match, int invert, float* dst, int cap_rows, int32_t* cursor_dev,
                            void* ws, size_t ws_bytes, void* stream);
/* dst[:, 0:2] = fp32(rotation of (x, y) in fp64 by (cosv, sinv)), z and column 3 copied, columns >= 4 zeroed */
int toda_points_rotate_z(const float* src, int n, const int32_t* n_dev, int c, double cosv, double sinv,
                         float* dst, void* stream);
/* Global augmentations in one pass, in the reference's order and fp32 arithmetic (pcdet/datasets/augmentor/
 * augmentor_utils.py:8-81 random_flip_along_x / _y, global_rotation, global_scaling): flip_x: y -> -y; flip_y: x -> -x;
 * rotate: (x, y) -> (x c - y s, x s + y c); rescale: xyz *= scale.  dst may alias src. */
int toda_points_world_transform(const float* src, int n, const int32_t* n_dev, int c, int flip_x, int flip_y,
                                int rotate, float cosv, float sinv, int rescale, float scale, float* dst,
                                void* stream);

/* ------------------------------------------------------------------------
 * Per-object and pyramid augmentations (pcdet/datasets/augmentor/augmentor_utils.py:124-683): the reference's Python loop
 * over the boxes, each iteration several numpy passes over the cloud, becomes one pass in which a thread carries its
 * point through every box in order.
 * ---------------------------------------------------------------------- */
/* steps: device double [n_steps, 10] rows (cx cy cz dx dy dz rz op p0 p1), in the order the reference visits them; the
 * box is the one the reference tested (get_points_in_box: 0.1 m margin in local x / y, none in z, borders included, fp32)
 * and is rounded to fp32.  For every row: walk the steps; where the row's CURRENT x, y, z lie in the step's box - or for
 * every row when op has bit 16 set - apply op & 15:
 *   0 / 1 / 2  x / y / z = fp32(fp64(v) + p0)                      3  rotate about z round the box centre, cos = p0, sin = p1 (fp32)
 *   4          v = (v - centre) * fp32(p0) + centre, v = x, y, z    5 / 6  drop if z >= p0 / z <= p0     7 / 8  drop if y >= p0 / y <= p0
 * A dropped row takes no further part.  dst rows get the new x, y, z and the other columns copied (dst may alias src;
 * rows in [min(n, *n_dev), n) are copied unchanged); keep (nullable, int32 [n]): 1 for a surviving valid row, else 0.
 * The table is staged through LDS in chunks of toda_points_box_steps_chunk() steps, n_steps is unbounded. */
int toda_points_box_steps_chunk(void);
int toda_points_box_steps(const float* src, int n, const int32_t* n_dev, int c, const double* steps, int n_steps,
                          float* dst, int32_t* keep, void* stream);
/* range_dev[0:2] = min, max of column col over the valid rows; deterministic.  A reduction always has a result: with no
 * valid row, n == 0 included, it writes (+inf, -inf) (as toda_points_pitch_range; points may be NULL only then).  NaN entries
 * are skipped (fminf / fmaxf), where numpy's min / max propagate them. */
size_t toda_points_column_range_workspace_bytes(void);
int toda_points_column_range(const float* points, int n, const int32_t* n_dev, int c, int col, float* range_dev,
                             void* ws, size_t ws_bytes, void* stream);
/* pyramids: device double [np, 5, 3] (apex, four base corners in order round the face: get_pyramids' layout).  A row is
 * inside when it satisfies the five half-spaces (fp64, faces included) - box_utils.in_hull's answer away from the faces.
 * bits: uint32 [n, ceil(np / 32)], bit p % 32 of word p / 32 = row in pyramid p (0 for rows beyond *n_dev);
 * counts: int32 [np], zeroed and filled by the call (integer atomics). */
int toda_points_in_pyramids(const float* points, int n, const int32_t* n_dev, int c, const double* pyramids, int np,
                            uint32_t* bits, int32_t* counts, void* stream);

/* Camera field-of-view test of a KITTI frame (csrc/kitti_frame.hip): flags[j] = 1 iff point j projects into the image with
 * non-negative depth (pcdet/datasets/kitti/kitti_dataset.py get_fov_flag + pcdet/utils/calibration_kitti.py lidar_to_rect /
 * rect_to_img):
 *   rect = [x y z 1] . M            M = fp32(V2C^T . R0^T), 4 x 3 row-major, formed on the host in fp32 as the reference forms it
 *   hom  = [rect 1] . P2^T          u = hom0 / rect_z, v = hom1 / rect_z, depth = hom2 - P2[2][3]      (P2: 3 x 4 row-major)
 *   flag = 0 <= u < img_w  and  0 <= v < img_h  and  depth >= 0        (fp32; NaN / inf compare false, as in numpy)
 * Rows, n_dev and flags as in the family above.  m_host and p2_host are host arrays of 12 floats, passed to the kernel by
 * value: no device upload, no sync.  Rows beyond min(n, *n_dev) are left untouched.  c < 3, n < 0, a null matrix, a
 * non-positive image size, or null points / flags with n > 0 return -1; n == 0 succeeds without a launch. */
int toda_points_fov_flags(const float* points, int n, const int32_t* n_dev, int c, const float* m_host,
                          const float* p2_host, int img_h, int img_w, int32_t* flags, void* stream);

/* Multi-sweep merge of a nuScenes sample (csrc/nuscenes_frame.hip; pcdet/datasets/nuscenes/nuscenes_dataset.py get_sweep /
 * get_lidar_with_sweeps): one pass over the concatenated raw rows of the sample's n_sweeps files, sweep 0 being the key frame.
 *   rows [n, 5] fp32 (x, y, z, intensity, ring), device; sweep s holds rows offsets_host[s] .. offsets_host[s + 1] - 1
 *   flags[j] = !(drop_ego[s] && |x| < radius && |y| < radius)       raw fp32 coordinates, strict, a NaN keeps the row
 *   x' = (float)(((double)x * m[0] + (double)y * m[1] + (double)z * m[2]) + m[3]), y' from m[4..7], z' from m[8..11]
 *        when has_matrix[s] (m = matrices_host + 12 s, a 3 x 4 row-major double matrix); x, y, z unchanged otherwise
 *   x', y', z' += shift_host[0..2] in fp32, after that rounding, when shift_host is not null
 *   out[j] = (x', y', z', intensity, (float)time_lags_host[s])       [n, 5] fp32, written for every row, kept or not
 * Every *_host argument is a host array (offsets n_sweeps + 1 int32, matrices 12 n_sweeps doubles, has_matrix / drop_ego
 * n_sweeps int32, time_lags n_sweeps doubles) and reaches the kernel by value: no device upload, no sync.  flags feed
 * toda_rows_select_append, which keeps the order: key frame, then the sweeps in table order, each in file order.
 * n < 0, n_sweeps outside 1 .. toda_sweeps_merge_max_sweeps(), a null table, a radius that is negative or NaN, offsets that
 * do not run from 0 to n without decreasing, or null rows / out / flags with n > 0 return -1; n == 0 succeeds without a launch. */
int toda_sweeps_merge_max_sweeps(void);
int toda_sweeps_merge(const float* rows, int n, int n_sweeps, const int32_t* offsets_host, const double* matrices_host,
                      const int32_t* has_matrix_host, const int32_t* drop_ego_host, const double* time_lags_host,
                      float radius, const float* shift_host, float* out, int32_t* flags, void* stream);

/* toda_sweeps_merge with an ego cut of two half-sides (the Lyft sample, pcdet/datasets/lyft/lyft_dataset.py remove_ego_points:
 * 1.5 m x 1.0 m): the same kernel and the same arguments, except that
 *   flags[j] = !(drop_ego[s] && |x| < radius_x && |y| < radius_y)   raw fp32 coordinates, strict, a NaN keeps the row
 * toda_sweeps_merge(radius) is toda_sweeps_merge_rect(radius, radius), bit for bit.  The same argument errors, a half-side that
 * is negative or NaN among them, return -1; n == 0 succeeds without a launch. */
int toda_sweeps_merge_rect(const float* rows, int n, int n_sweeps, const int32_t* offsets_host, const double* matrices_host,
                           const int32_t* has_matrix_host, const int32_t* drop_ego_host, const double* time_lags_host,
                           float radius_x, float radius_y, const float* shift_host, float* out, int32_t* flags, void* stream);

/* Point pass of a processed Waymo frame (csrc/waymo_frame.hip; pcdet/datasets/waymo/waymo_dataset.py get_lidar):
 *   rows [n, c_in] fp32, device, c_in >= 6: x, y, z, intensity, elongation, NLZ flag (further columns are not read)
 *   out[j]   = (x, y, z, (float)tanh((double)intensity), elongation)  [n, 5] fp32, written for every row, kept or not; the fp64
 *              routine rounded once: the sign of zero stays, a NaN passes, large values give +-1
 *   flags[j] = use_nlz ? row[5] == -1.0f : 1                            int32; a NaN or a neighbour of -1 gives 0; with
 *              use_nlz == 0 column 5 is not read
 * flags feed toda_rows_select_append, which keeps the file order.  n < 0, c_in < 6, or null rows / out / flags with n > 0 return
 * -1; n == 0 succeeds without a launch. */
int toda_waymo_frame(const float* rows, int n, int c_in, int use_nlz, float* out, int32_t* flags, void* stream);

/* Adversarial edit of one pseudo-labelled frame (csrc/adv_frame.hip; pcdet/datasets/nuscenes/nuscenes_mixup_adv_dataset.py
 * get_ps_adv_lidar_with_sweeps, :191-274).
 *   points [n, c] fp32, device, c >= 4: x, y, z, then the rest
 *   table  [k, 10] doubles (cx cy cz dx dy dz rz op frac seed), once on the host (table_host: checked before anything is
 *          launched) and once on the device (table_dev: what the kernels read); the box is rounded to fp32;
 *          op 0 modify, 1 add, 2 remove, 3 nothing; frac in [0, 1); seed an integer below 2^32.
 *          Contract: table_dev holds the same k * 10 doubles as table_host - the caller uploads the table it had checked
 *          (ops.adv_edit builds one array and passes both).  The entry point cannot compare the two without a read-back, so
 *          only table_host is validated; in a device copy that differs, an op outside 0..2 does not act, frac is clamped to
 *          k_j in [0, c_j - 1] and the seed is converted to uint32 unchecked: a wrong edit, never an access out of bounds.
 *   keys   [m] int64, device, sorted: linear voxel index (z * gy + y) * gx + x;   grads [m, 3] fp32, device
 *   range_lo_host[3], voxel_host[3], grid_host[3] (x, y, z) and eps reach the kernels by value
 * Row i:  g_i = grads[pos] where keys[pos] == key of cell floor((xyz - range_lo) / voxel) (fp32 subtraction and division), zero
 *         outside the grid, for an absent key and with m == 0;  d_i = eps * g_i in fp32.
 * Box j:  S_j = rows whose ORIGINAL x, y, z pass get_points_in_box (mode 1 of toda_points_in_boxes), c_j = |S_j|.  It acts when
 *         op is 0 or 1 and c_j >= 1, or op is 2 and c_j > 5.  Then k_j = min(floor(frac * c_j), c_j - 1) (fp64 product) and T_j =
 *         the c_j - k_j rows of S_j smallest in key_j(i) = fmix32(seed ^ uint32(i * 0x9E3779B9)) (murmur3's 32-bit finaliser;
 *         the keys of a box differ pairwise).  Otherwise T_j is empty.
 * A row walks the boxes in table order with cur = its original x, y, z; for i in T_j: modify cur -= d_i; add emits a row
 * (cur - d_i, the other columns of row i); remove marks the row (it still takes part in later boxes).
 * Output at dst[*cursor_dev ...]: the unmarked rows in order with their final cur, then the emitted rows in (i, j) order;
 * *cursor_dev += their number; rows beyond cap_rows are dropped (the cursor still counts them, as toda_rows_select_append).
 * counts [k] int32 = c_j.  A row with a NaN coordinate lies in no box and passes through.
 * n == 0 or k == 0 succeed without a launch and write nothing: with k == 0 the output is the input.  c < 4, k above
 * toda_adv_edit_max_boxes(), n * (k + 1) >= 2^31, a null host array, non-positive voxel or grid sizes, an op outside 0..3, a frac
 * outside [0, 1), a seed that is no uint32, a workspace below toda_adv_edit_workspace_bytes(n, k) or a null device pointer return
 * an error, in this order, before anything is launched.  The table is staged through LDS toda_adv_edit_chunk() boxes at a time. */
int toda_adv_edit_max_boxes(void);
int toda_adv_edit_chunk(void);
size_t toda_adv_edit_workspace_bytes(int n, int k);
int toda_adv_edit(const float* points, int n, int c, const double* table_host, const double* table_dev, int k,
                  const int64_t* keys, const float* grads, int m, const float* range_lo_host, const float* voxel_host,
                  const int32_t* grid_host, float eps, float* dst, int cap_rows, int32_t* cursor_dev, int32_t* counts,
                  void* ws, size_t ws_bytes, void* stream);

/* Forward convolution that also returns the BatchNorm statistics of its output (reference
 * pcdet/models/backbones_3d/spconv_backbone.py:21-25,54-64: every sparse conv is followed by BatchNorm1d): the
 * per-channel sum and sum of squares are taken from the accumulators in the kernel's epilogue, so the separate
 * statistics pass over the output (toda_rows_moments) disappears.  sums: toda_spconv_gather_gemm_stats_doubles()
 * doubles; on return sums[0:c] = sum, sums[c:2c] = sum of squares (the layout toda_bn_finalize reads; fixed-order
 * fold, deterministic).  Only for channel pairs toda_spconv_gather_gemm_stats_supported() accepts. */
int toda_spconv_gather_gemm_stats_supported(int c_gather, int c_produce);
size_t toda_spconv_gather_gemm_stats_doubles(int n_out, int c_produce);
int toda_spconv_gather_gemm_stats(const float* in, int n_in, int c_gather, const float* packed_w, const int32_t* nbr,
                                  int n_out, int k_vol, int c_produce, const float* bias, float* out, double* sums,
                                  size_t sums_doubles, void* stream);
/* toda_spconv_gather_gemm_stats without the fold of the partial sums: *blocks_out (host memory, written before the call returns)
 * = number of partials per column, to be handed to toda_bn_finalize_partials. */
int toda_spconv_gather_gemm_stats_partials(const float* in, int n_in, int c_gather, const float* wp, const int32_t* nbr,
                                           int n_out, int k_vol, int c_produce, const float* bias /*nullable*/, float* out,
                                           double* sums, size_t sums_doubles, int* blocks_out, void* stream);

/* ------------------------------------------------------------------------
 * Dense 3x3 / stride 1 / pad 1 fp32 convolution of the BEV neck and the dense heads (NCHW), replacing
 * torch.nn.Conv2d -> cuDNN / MIOpen at pcdet/models/backbones_2d/base_bev_backbone.py:37-58,81-112 and
 * pcdet/models/dense_heads/center_head.py:20-28,73-80 together with autograd's backward of those layers
 * (tools/train_utils/train_utils.py:55).  Fused Winograd F(4x4,3x3) on the fp32 matrix cores; nothing of the
 * Winograd domain is written to memory.  w is torch's [Cout][Cin][3][3].
 *   toda_conv3x3_supported        1 when (batch, cin, cout, H, W) can run here in all three directions
 *                                 (channels multiples of 32, W even, tensors below 4 GiB), else 0
 *   toda_conv3x3_transform_weight u = G w G^T in the kernel's operand order; mode 0: forward,
 *                                 mode 1: data gradient (filters rotated by 180 degrees, channel roles swapped),
 *                                 mode 2: both, forward operand first (2 x toda_conv3x3_weight_floats floats)
 *   toda_conv3x3_transform_weight_batch  the same for n layers in one launch (16 layers per launch): table is a HOST
 *                                 array of {w, cout, cin, mode, u} entries; every u[i] gets the bits the per-layer call
 *                                 writes.  Once per step for the stride-1 3x3 layers of a dense stack.
 *   toda_conv3x3_fwd              y[B][cout][H][W] = conv(x[B][cin][H][W]) (+ bias[cout], nullable).  With the
 *                                 mode-1 operand and (cin, cout) = (Cout, Cin) of the layer it computes dX from dY.
 *                                 ws: toda_conv3x3_workspace_bytes() bytes, ZERO before the first call and used by
 *                                 one call at a time (hand-off flags, which every call leaves zero again, +
 *                                 partial-sum slabs of the stream-K work split)
 *   toda_conv3x3_wgrad            dw[Cout][Cin][3][3] from x and dy (workspace: per-split partial sums, folded
 *                                 in fixed order - deterministic, no float atomics).  The fold and G^T . G are one
 *                                 kernel; TODA_WGRAD_FOLD=pair runs them as two with the per-unit sums in the
 *                                 workspace between them (same bits).
 * ---------------------------------------------------------------------- */
int toda_conv3x3_supported(int batch, int cin, int cout, int H, int W);
size_t toda_conv3x3_weight_floats(int cout, int cin);
int toda_conv3x3_transform_weight(const float* w, int cout, int cin, int mode, float* u, void* stream);
typedef struct toda_conv3x3_weight_entry {
    const float* w; /* [cout][cin][3][3] */
    int32_t cout, cin, mode, reserved;
    float* u;       /* toda_conv3x3_weight_floats(cout, cin) floats, twice that for mode 2 */
} toda_conv3x3_weight_entry;
int toda_conv3x3_transform_weight_batch(const toda_conv3x3_weight_entry* table_host, int n, void* stream);
size_t toda_conv3x3_workspace_bytes(void);
size_t toda_conv3x3_wgrad_workspace_bytes(int batch, int cin, int cout, int H, int W);
int toda_conv3x3_wgrad(const float* x, const float* dy, int batch, int cin, int cout, int H, int W, float* dw,
                       void* ws, size_t ws_bytes, void* stream);
int toda_conv3x3_fwd(const float* x, const float* u, const float* bias, int batch, int cin, int cout, int H,
                     int W, float* y, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The other convolutions of BaseBEVBackbone (pcdet/models/backbones_2d/base_bev_backbone.py:32-36: ZeroPad2d(1) +
 * Conv2d(c_in, c, 3, stride 2, padding 0) at the head of a block; :47-66: the deblocks ConvTranspose2d(c, c_up, k = s,
 * stride = s) with s = 1 and s = 2), forward and autograd backward on the fp32 matrix cores, NCHW in and out (torch runs them
 * on MIOpen / rocBLAS behind layout transposes and im2col / col2im passes).
 *   toda_conv3x3s2_*   x [B][cin][H][W] (H, W even) -> y [B][cout][H/2][W/2]; w [cout][cin][3][3] (nn.Conv2d layout).
 *                      _dgrad covers the four input-pixel parities in one launch (an input pixel is reached by 1, 2, 2 or 4 of
 *                      the 9 taps); _wgrad contracts over pixels in splits, folded in fixed order (deterministic).
 *   toda_deconv_*      x [B][cin][H][W] -> y [B][cout][s H][s W]; w [cin][cout][s][s] (nn.ConvTranspose2d layout), s in {1, 2};
 *                      the pixel shuffle of s = 2 is the store of the forward GEMM / the gather of the backward ones.
 * No bias (the reference builds these layers with bias=False; a caller with a bias adds it afterwards).
 * ---------------------------------------------------------------------- */
int toda_conv3x3s2_supported(int batch, int cin, int cout, int H, int W);
int toda_conv3x3s2_fwd(const float* x, const float* w, int batch, int cin, int cout, int H, int W, float* y, void* stream);
int toda_conv3x3s2_dgrad(const float* dy, const float* w, int batch, int cin, int cout, int H, int W, float* dx, void* stream);
size_t toda_conv3x3s2_wgrad_workspace_bytes(int batch, int cin, int cout, int H, int W);
int toda_conv3x3s2_wgrad(const float* x, const float* dy, int batch, int cin, int cout, int H, int W, float* dw, void* ws,
                         size_t ws_bytes, void* stream);
int toda_deconv_supported(int batch, int cin, int cout, int H, int W, int s);
int toda_deconv_fwd(const float* x, const float* w, int batch, int cin, int cout, int H, int W, int s, float* y, void* stream);
int toda_deconv_dgrad(const float* dy, const float* w, int batch, int cin, int cout, int H, int W, int s, float* dx, void* stream);
size_t toda_deconv_wgrad_workspace_bytes(int batch, int cin, int cout, int H, int W, int s);
int toda_deconv_wgrad(const float* x, const float* dy, int batch, int cin, int cout, int H, int W, int s, float* dw, void* ws,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * CenterHead.get_loss of one head group, value and gradient (pcdet/models/dense_heads/center_head.py:229-262:
 * sigmoid + clamp(1e-4, 1 - 1e-4) of the heat-map logits; pcdet/utils/loss_utils.py:264-297 neg_loss_cornernet /
 * FocalLossCenterNet; :300-385 _gather_feat, _transpose_and_gather_feat, _reg_loss / RegLossCenterNet; the
 * code_weights / loc_weight / cls_weight products of center_head.py:250-257).
 *   hm_logits, heatmap [B][classes][H][W]; reg_maps_host[] = n_branch device pointers [B][c_j][H][W] in HEAD_ORDER
 *   (sum c_j = code_size <= 16); inds, mask [B][max_objs] int64; target_boxes [B][max_objs][code_size];
 *   code_weights: HOST array.
 *   _fwd  hm_prob = clamped sigmoid; out4 = {hm_loss * cls_weight, loc_loss * loc_weight, 1 / max(num_pos, 1),
 *         1 / max(num_objs, 1)} (device); ws keeps what _bwd needs (the same ws must be passed on)
 *   _bwd  up_hm / up_loc: device scalars dL/d(out4[0]), dL/d(out4[1]); hm_grad [B][classes][H][W];
 *         reg_grads_host[]: gradient maps of the branches (zero-filled here, then scattered into)
 * Sums are folded in a fixed order (fp64 partials): no atomics, bitwise reproducible.
 * ---------------------------------------------------------------------- */
size_t toda_center_loss_workspace_bytes(int batch, int classes, int H, int W, int max_objs, int code_size);
int toda_center_loss_fwd(const float* hm_logits, const float* heatmap, int batch, int classes, int H, int W, int n_branch,
                         const float* const* reg_maps_host, const int32_t* reg_channels_host, const int64_t* inds,
                         const int64_t* mask, const float* target_boxes, int max_objs, int code_size,
                         const float* code_weights_host, float cls_weight, float loc_weight, float* hm_prob, float* out4,
                         void* ws, size_t ws_bytes, void* stream);
int toda_center_loss_bwd(const float* out4, const float* up_hm, const float* up_loc, int batch, int classes, int H, int W,
                         int n_branch, float* const* reg_grads_host, const int32_t* reg_channels_host, const int64_t* inds,
                         const int64_t* mask, int max_objs, int code_size, const float* code_weights_host, float cls_weight, float loc_weight,
                         float* hm_grad, const void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 convolutions with 1..4 OUTPUT channels: the last layer of every CenterHead branch
 * (pcdet/models/dense_heads/center_head.py:20-28: Conv2d(64, out_channels, 3, padding=1, bias=True) of center /
 * center_z / dim / rot / hm), forward and autograd backward.  All n <= 8 branches of a head go through ONE launch
 * per direction.  Pointer arguments ending in [] are HOST arrays of n device pointers, cout_host holds the n
 * output-channel counts; every branch has the same (batch, cin, H, W), W % 4 == 0, W <= 256.  x_image_stride /
 * dx_image_stride: floats between two images of a branch input (its gradient): 0 = dense (cin * H * W); larger when
 * the branch inputs are channel slices of one [B][n * cin][H][W] tensor (the fused hidden layer of the head).
 *   _fwd     y_i[B][cout_i][H][W] = conv(x_i[B][cin][H][W], w_i[cout_i][cin][3][3]) + bias_i (bias_host may be NULL)
 *   _dgrad   dx_i[B][cin][H][W] from dy_i and w_i
 *   _wgrad   out = for i in order: dw_i [cout_i][cin][3][3] then db_i [cout_i]  (band slabs in ws, fixed-order fold)
 * ---------------------------------------------------------------------- */
int toda_conv3x3_narrow_supported(int batch, int cin, int cout, int H, int W);
int toda_conv3x3_narrow_fwd(int n, const float* const* x_host, const float* const* w_host, const float* const* bias_host,
                            const int32_t* cout_host, int batch, int cin, int H, int W, long long x_image_stride,
                            float* const* y_host, void* stream);
int toda_conv3x3_narrow_dgrad(int n, const float* const* dy_host, const float* const* w_host, const int32_t* cout_host,
                              int batch, int cin, int H, int W, long long dx_image_stride, float* const* dx_host, void* stream);
size_t toda_conv3x3_narrow_wgrad_workspace_bytes(int n, int batch, int cin, int H);
int toda_conv3x3_narrow_wgrad(int n, const float* const* x_host, const float* const* dy_host, const int32_t* cout_host,
                              int batch, int cin, int H, int W, long long x_image_stride, float* out, void* ws, size_t ws_bytes,
                              void* stream);

/* ------------------------------------------------------------------------
 * Instrumentation (no counterpart in the reference): per-launch durations of the gather-GEMM kernels, taken
 * from start / stop events stamped on the kernel dispatch itself (hipExtLaunchKernelGGL), i.e. the number
 * rocprofv3 --kernel-trace reports.  toda_timing_begin arms up to `capacity` launches of
 * toda_spconv_gather_gemm (process-wide, one stream at a time); toda_timing_end waits for them and returns the
 * milliseconds in launch order (*n_out = launches seen).
 * ---------------------------------------------------------------------- */
int toda_timing_begin(int capacity);
int toda_timing_end(float* ms_out_host, int cap, int* n_out_host);

/* ---------------------------------------------------------------------------------------------
 * The optimizer step of the reference trainers in two launches (reference tools/train_utils/train_utils.py:55-59:
 * clip_grad_norm_(model.parameters(), GRAD_NORM_CLIP) + optimizer.step(), the optimizer being
 * tools/train_utils/optimization/fastai_optim.py:104-236 OptimWrapper(Adam, true_wd) = p *= 1 - lr * wd, then torch's Adam):
 *   norm = || all gradients ||_2 (returned in norm_out[0]); g *= min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping);
 *   p *= 1 - lr * weight_decay; m += (g - m)(1 - beta1); v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).
 * The n tensors (fp32, contiguous) are given as device arrays of device addresses + element counts; chunk_tensor / chunk_off list
 * the toda_clip_adam_chunk()-element pieces of all tensors (one workgroup each); partial: n_chunks doubles of scratch.  The partial
 * sums are folded in index order: deterministic. */
int toda_clip_adam_chunk(void);
int toda_clip_adam_step(const unsigned long long* param, const unsigned long long* grad, const unsigned long long* exp_avg,
                        const unsigned long long* exp_avg_sq, const long long* numel, const int* chunk_tensor,
                        const long long* chunk_off, int n_chunks, double* partial, float* norm_out, float max_norm,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The device parts of the KITTI AP evaluator (reference pcdet/datasets/kitti/kitti_object_eval_python: rotate_iou.py, a
 * numba-CUDA kernel, and eval.py:87-154 image_box_overlap / d3_box_overlap, eval.py:157-337 compute_statistics_jit /
 * fused_compute_statistics, numba-JIT host loops).  Boxes and queries of F frames are given flat with CSR offsets
 * (int32 [F + 1]); only same-frame pairs are computed.
 *
 * toda_eval_overlaps: out + out_off[f] holds frame f's [n_box_f, n_query_f] block, row major, fp32 (out_off: int64 [F + 1],
 * n_pairs = out_off[F]).  box3d / query3d rows: x, y, z, l, h, w, rotation_y in the KITTI camera frame (y the bottom face);
 * bbox / query_bbox rows: x1, y1, x2, y2; the set a metric does not read may be NULL.
 *   metric 0  image boxes            criterion -1: inter / union, 0: / box area, 1: / query area, 2: / 1
 *   metric 1  BEV rectangles (x, z, l, w, ry): exact clipping with no corner margin, angles clockwise-positive, fp32;
 *             the reference hands its device function the QUERY first, so criterion 0: / query area, 1: / box area,
 *             2: the intersection area
 *   metric 2  BEV intersection x overlap of [y - h, y]; criterion 0: / box volume, 1: / query volume, 2: / itself
 *
 * toda_eval_match: for one (class, difficulty, min_overlap, metric) the greedy assignment of every frame at every one of the
 * n_thresh score thresholds, pr[n_thresh, 4] = (tp, fp, fn, AOS similarity) summed over the frames in a fixed order (two
 * runs: same bits).  overlaps / ov_off as written by toda_eval_overlaps with the detections as boxes and the ground truths
 * as queries; ign_det / ign_gt: -1 another class, 0 counts, 1 ignored; det_bbox [n_det, 4], dc_bbox / dc_off (DontCare
 * regions per frame) are read for metric 0 only, the alphas only with compute_aos.
 * toda_eval_match_scores: the threshold-free first pass: scores_out[gt_off[f] + k], k < count_out[f], are the scores of the
 * detections matched to frame f's counted ground truths, in ground-truth order.
 * ws: toda_eval_match_workspace_bytes(n_frames, n_thresh, n_det_total) bytes (n_thresh = 1 for _scores).
 * ---------------------------------------------------------------------- */
int toda_eval_overlaps(const float* box3d, const float* bbox, const int32_t* box_off, const float* query3d,
                       const float* query_bbox, const int32_t* query_off, const long long* out_off, int n_frames,
                       long long n_pairs, int metric, int criterion, float* out, void* stream);
size_t toda_eval_match_workspace_bytes(int n_frames, int n_thresh, int n_det_total);
int toda_eval_match_scores(const float* overlaps, const long long* ov_off, const int32_t* det_off, const int32_t* gt_off,
                           const int32_t* ign_det, const int32_t* ign_gt, const double* det_score, int n_frames,
                           int n_det_total, double min_overlap, double* scores_out, int32_t* count_out, void* ws,
                           size_t ws_bytes, void* stream);
int toda_eval_match(const float* overlaps, const long long* ov_off, const int32_t* det_off, const int32_t* gt_off,
                    const int32_t* ign_det, const int32_t* ign_gt, const double* det_score, const double* det_alpha,
                    const double* gt_alpha, const double* det_bbox, const double* dc_bbox, const int32_t* dc_off, int n_frames,
                    int n_det_total, const double* thresholds, int n_thresh, double min_overlap, int metric, int compute_aos,
                    double* pr, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The device parts of the nuScenes detection metric (mAP / NDS, public definition `detection_cvpr_2019`; the reference hands
 * the metric to the nuScenes devkit).  fp64 throughout, no atomics: two runs give the same bits.  Classes are numbered in
 * the order car, truck, bus, trailer, construction_vehicle (range 50 m), pedestrian, motorcycle, bicycle (40 m),
 * traffic_cone, barrier (30 m).
 *
 * toda_nusc_eval_prepare: n LiDAR-frame boxes, predictions or ground truths, to the global frame.  rows [n, 10] = x y z dx dy
 * dz heading vx vy vz; sample [n] indexes G [n_samples, 12] (row-major 3 x 4, G = inv(car_from_global) . inv(ref_from_car))
 * and ego [n_samples, 3] (the translation of inv(car_from_global)); cls [n] is the class number, anything outside 0..9 is
 * never kept.  out [n, 6] = centre x y z, yaw, velocity x y; keep [n] = 1 iff the xy distance from the centre to ego is
 * strictly below the class's range.  A row whose sample index lies outside [0, n_samples) gets NaN and keep 0.
 *
 * toda_nusc_eval_match: the greedy centre-distance matching of every (sample, class) segment at the four thresholds.
 * pred / gt rows [., 8] = centre x y, yaw, velocity x y, dx dy dz, stored segment after segment; pred_off_host / gt_off_host
 * (HOST, int32 [n_seg + 1]) are the CSR offsets of both sides and seg_cls_host (HOST, int32 [n_seg]) the class number of
 * each segment; they are checked and copied into ws.  A segment holds at most TODA_NUSC_MAX_PRED predictions (the metric's
 * own limit per sample) and TODA_NUSC_MAX_GT ground truths (64 lanes x the 32 bits of a lane's taken mask); more is refused.
 * Predictions are visited by (score descending, position descending); each takes the nearest free ground truth of its segment
 * (lowest position on equal distances) iff that distance is strictly below the threshold.  match [4, n_pred]: the row of the
 * ground truth in gt, or -1.  err [5, n_pred], written for thresholds_host[tp_threshold] only: translation, velocity (NaN
 * with a NaN ground-truth velocity), 1 - IoU of the centre-aligned sizes, yaw difference (period pi for barriers) and
 * attribute (0 equal, 1 different, NaN when gt_attr < 0); NaN where unmatched.
 * ws: toda_nusc_eval_match_workspace_bytes(n_seg) bytes.
 * ---------------------------------------------------------------------- */
#define TODA_NUSC_MAX_PRED 500
#define TODA_NUSC_MAX_GT 2048
int toda_nusc_eval_prepare(const double* rows, const int32_t* sample, const int32_t* cls, int n, const double* G,
                           const double* ego, int n_samples, double* out, int32_t* keep, void* stream);
size_t toda_nusc_eval_match_workspace_bytes(int n_seg);
int toda_nusc_eval_match(const double* pred, const double* pred_score, const int32_t* pred_attr, int n_pred, const double* gt,
                         const int32_t* gt_attr, int n_gt, const int32_t* pred_off_host, const int32_t* gt_off_host,
                         const int32_t* seg_cls_host, int n_seg, const double* thresholds_host, int tp_threshold,
                         int32_t* match, double* err, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The device parts of the Waymo detection metric (LEVEL_1 / LEVEL_2 AP and APH per object type; the reference
 * hands the metric to TensorFlow and the waymo_open_dataset package).  fp64 and integers throughout, no float atomics: two
 * runs give the same bits.  A segment is one (frame, object type); boxes [., 7] = x y z dx dy dz heading are stored segment
 * after segment.  pred_off_host / gt_off_host (HOST, int32 [n_seg + 1]) are the CSR offsets of both sides, iou_off_host
 * (HOST, int64 [n_seg + 1]) those of the segments' [n_pred_s, n_gt_s] row-major IoU blocks, n_pairs = iou_off_host[n_seg].
 * They are checked on the host (null, negative, descending, a block that is not n_pred_s x n_gt_s, a segment over
 * TODA_WAYMO_MAX_PRED predictions or TODA_WAYMO_MAX_GT ground truths: refused before anything is launched) and copied into ws.
 *
 * toda_waymo_eval_iou: the 7-DOF IoU of every same-segment pair.  Exact convex clipping of the prediction's rectangle by the
 * four half-planes of the ground truth's, no corner margins; shoelace area times the overlap of the z-intervals;
 * inter / (volA + volB - inter), 0 when that denominator is not positive, clamped to [0, 1].
 *
 * toda_waymo_eval_match: per segment and score cutoff the maximum-weight one-to-one assignment between the predictions with
 * (fp32) score >= cutoff and the ground truths, on the weights w = IoU >= t ? (int)(IoU * 1000) : 0 with t = 0.7 for type 1
 * (Vehicle) and 0.5 for types 2..4 (Pedestrian, Sign, Cyclist); a pair is a match iff it is assigned and w > 0.  Where the
 * optimum is not unique, which optimal assignment is returned is not specified.  seg_type_host (HOST, int32 [n_seg]) holds
 * 1..4; cutoffs_host (HOST, fp32 [TODA_WAYMO_CUTOFFS]) must ascend; gt_level [n_gt] is the difficulty, a ground truth is in
 * level L iff it is <= L.  Summed over the segments of a type in a fixed order:
 *   tp, fn  int64 [4, 2, 101]   matched / unmatched ground truths in level (type - 1, level - 1, cutoff)
 *   fp      int64 [4, 101]      unmatched active predictions (one matched to a ground truth above the level counts nowhere)
 *   sum_ha  fp64  [4, 2, 101]   over the TPs: 1 - min(d, 2 pi - d) / pi, d = |heading difference| mod 2 pi
 * match_dbg (may be NULL): int32 [101, n_pred], at every cutoff the row in the ground-truth arrays each prediction is matched
 * to, -1 when unmatched or inactive.
 * ws: toda_waymo_eval_match_workspace_bytes(n_seg) bytes, for either call.
 * ---------------------------------------------------------------------- */
#define TODA_WAYMO_MAX_PRED 512
#define TODA_WAYMO_MAX_GT 512
#define TODA_WAYMO_CUTOFFS 101
size_t toda_waymo_eval_match_workspace_bytes(int n_seg);
int toda_waymo_eval_iou(const double* pred, int n_pred, const double* gt, int n_gt, const int32_t* pred_off_host,
                        const int32_t* gt_off_host, const long long* iou_off_host, int n_seg, long long n_pairs, double* iou,
                        void* ws, size_t ws_bytes, void* stream);
int toda_waymo_eval_match(const double* iou, const float* pred_score, const double* pred_heading, int n_pred,
                          const double* gt_heading, const int32_t* gt_level, int n_gt, const int32_t* pred_off_host,
                          const int32_t* gt_off_host, const long long* iou_off_host, const int32_t* seg_type_host, int n_seg,
                          long long n_pairs, const float* cutoffs_host, long long* tp, long long* fn, long long* fp,
                          double* sum_ha, int32_t* match_dbg, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The device parts of the Lyft detection metric (mAP over ascending IoU cut-offs; reference
 * pcdet/datasets/lyft/lyft_mAP_eval/lyft_eval.py get_average_precisions).  fp64 and integers throughout, no atomics: two runs
 * give the same bits.  A segment is one (sample, class); both sides are stored segment after segment as rows of 8 doubles in
 * the global frame: centre x y z, c, s, width, length, height, where (c, s) is the first column of the box's rotation and is
 * NOT normalised.  The ground rectangle is centre +- length / 2 (c, s) +- width / 2 (s, -c), the volume width * length * height.
 * pred_off_host / gt_off_host (HOST, int32 [n_seg + 1]) are the CSR offsets of both sides; they are checked on the host (null,
 * negative, descending, not running from 0 to the total: refused before anything is launched) and copied into ws.  A segment
 * has no size cap: the kernels walk a long side in chunks.
 *
 * toda_lyft_eval_best: for every prediction the largest IoU over the ground truths of its segment and the position within the
 * segment of the first ground truth that attains it (numpy's max / argmax); best_gt = -1 and best_iou = -inf in a segment
 * without ground truths.  IoU: the prediction's rectangle clipped exactly by the four edges of the ground truth's (no corner
 * margins), shoelace area, times the overlap of the z intervals, divided by volA + volB - inter, clamped to [0, 1].  Sizes must
 * be positive and every value finite (the caller's check).
 *
 * toda_lyft_eval_flags: tp [n_thresholds, n_pred] uint8.  Within a segment q stands before p iff score_q > score_p, or the
 * scores are equal and q is stored earlier (a stable descending sort).  With m_p the largest best_iou_q over the q before p
 * that have best_gt_q == best_gt_p (-inf when there is none),
 *   tp[t, p] = best_iou_p > thresholds[t] && !(m_p > thresholds[t])
 * which is the reference's sequential walk: a ground truth is claimed at t by the first prediction in that order whose largest
 * IoU exceeds t and falls on it.  A prediction is a false positive wherever it is not a true positive.  thresholds_host (HOST,
 * fp64) holds 1 .. TODA_LYFT_MAX_CUTOFFS strictly ascending values; score fp64 [n_pred] must hold no NaN (the caller's check).
 * toda_lyft_eval_flags_chunk(): the number of predictions of one LDS stage of that kernel.
 *
 * n_pred == 0 or n_seg == 0 succeeds without a launch.  ws: toda_lyft_eval_workspace_bytes(n_seg) bytes, for either call.
 * ---------------------------------------------------------------------- */
#define TODA_LYFT_MAX_CUTOFFS 16
int toda_lyft_eval_flags_chunk(void);
size_t toda_lyft_eval_workspace_bytes(int n_seg);
int toda_lyft_eval_best(const double* pred, int n_pred, const double* gt, int n_gt, const int32_t* pred_off_host,
                        const int32_t* gt_off_host, int n_seg, double* best_iou, int32_t* best_gt, void* ws, size_t ws_bytes,
                        void* stream);
int toda_lyft_eval_flags(const double* score, const double* best_iou, const int32_t* best_gt, int n_pred,
                         const int32_t* pred_off_host, int n_seg, const double* thresholds_host, int n_thresholds, uint8_t* tp,
                         void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The consistency term of the stage-2 step (reference pcdet/models/__init__.py get_consistency_loss): mutual
 * nearest-centre matching between the boxes of the adversarial and the original pass, and both loss terms, for a whole batch.
 * adv [batch, na, cols] and org [batch, no, cols] fp32 rows x y z dx dy dz ..., cols >= 6; adv_sel [batch, na] and org_sel
 * [batch, no] one byte per row, non-zero = the row takes part.  Unselected rows are never read.
 *   d2(i, j) = ((ax - ox)^2 + (ay - oy)^2) + (az - oz)^2 in fp32, in this order, no contraction.
 *   best(i) = min over the selected j, p(i) = the smallest j that attains it; a NaN distance counts as smaller than every
 *   number (a row that meets one has best = NaN and no partner); no selected j: best = +inf.  i is matched iff
 *   best(i) < match_dist2, strictly.  The same for every selected j over the selected i.
 *   centre_sum = sum over matched i, c < 3 of |a[i, c] - o[p(i), c]| + the same over matched j; size_sum: (. - .)^2 over
 *   columns 3..5.  n = max(1, selected adv + selected org).
 * out [2 + 4 * batch]: sum_b (centre_sum_b / n_b) / batch, sum_b (size_sum_b / n_b) / batch, then per sample centre_sum,
 * size_sum, selected, matched (counts as fp32).  No float atomics, every sum folded in a fixed order: two runs give the same
 * bits.  Two launches.  ws: toda_consistency_workspace_bytes(batch, na, no) bytes.
 * ---------------------------------------------------------------------- */
size_t toda_consistency_workspace_bytes(int batch, int na, int no);
int toda_consistency_loss(const float* adv, const uint8_t* adv_sel, int na, const float* org, const uint8_t* org_sel, int no,
                          int batch, int cols, float match_dist2, float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TODA_H_ */
