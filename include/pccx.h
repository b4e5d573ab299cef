/*
 * pccx.h -- C ABI of libpccx.so, the MI355X (gfx950) implementation of the
 * patch-based compress / decompress hot path of rhmes/point-cloud-compression.
 *
 * The reference has no FFI of its own: its hot path is a set of Python callables
 * (pn_kit.py, octree_np.py, AE.py) plus pytorch3d / torchac functions they import.
 * Each entry point below replaces one of those callables (cited as file:line
 * relative to the reference root).  INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - tensors are dense, row-major, fp32 / int32 / int64 / uint8 as declared;
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work,
 *     they never synchronise;
 *   - return value: 0 on success, otherwise a negative pccx_status; the text of the
 *     last error on the calling thread is returned by pccx_last_error().
 */
#ifndef PCCX_H
#define PCCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCCX_API __attribute__((visibility("default")))

typedef enum {
    PCCX_OK = 0,
    PCCX_ERR_ARG = -1,        /* bad shape / unsupported size */
    PCCX_ERR_HIP = -2,        /* a HIP runtime call failed */
    PCCX_ERR_UNSUPPORTED = -3
} pccx_status;

PCCX_API const char *pccx_last_error(void);
PCCX_API int pccx_version(void);

/* ---- geometry ---------------------------------------------------------------------------- */

/* pn_kit.normalize (pn_kit.py:47-60), batched: per cloud b, centre on the bounding-box
 * middle, scale the longest side to (1-margin), shift by +0.5.
 * pc,out: (B,N,3) f32 (may alias); center: (B,3); longest: (B). */
PCCX_API int pccx_normalize(const float *pc, int B, int N, double margin, float *out, float *center,
                            float *longest, void *stream);

/* pn_kit.denormalize (pn_kit.py:62-66). pc,out: (B,N,3). */
PCCX_API int pccx_denormalize(const float *pc, int B, int N, double margin, const float *center,
                              const float *longest, float *out, void *stream);

/* pn_kit.farthest_point_sample_batch (pn_kit.py:309-330) with the random start (:321) made an
 * explicit argument; also pytorch3d sample_farthest_points (pointnet_sa_module.py:12) with
 * start 0.  xyz: (B,N,3); start_idx: (B) int32 device, or NULL for start 0; idx_out: (B,npoint)
 * int64.  workspace: B*N floats, required only when N > 16384 (else may be NULL). */
PCCX_API int pccx_fps(const float *xyz, int B, int N, int npoint, const int32_t *start_idx,
                      int64_t *idx_out, float *workspace, void *stream);

/* The same indices, bit for bit, with every cloud shared by G workgroups of 1024 threads (one cooperative launch of B * G
 * workgroups; each keeps its share of the cloud and of the running minima in registers, the winners of a round meet in `workspace`
 * through agent-scope atomics and a bounded grid barrier over the cloud's G workgroups).  ceil(N / 16384) <= G <= 64, so
 * N <= 1048576, and B * G must not exceed the device's compute-unit count (all workgroups have to be resident): PCCX_ERR_ARG
 * otherwise, before anything is launched.  workspace: pccx_fps_coop_workspace_bytes(B, npoint) bytes on the device, cleared by the
 * entry itself; per cloud (npoint + 2) 64-bit words, word 1 of them the STATUS word: non-zero after the launch when a barrier wait
 * ran out of its bound (about a second) and the cloud's workgroups gave up -- idx_out of that cloud is then incomplete.  Not for
 * stream capture (the caller reads the status words). */
PCCX_API size_t pccx_fps_coop_workspace_bytes(int B, int npoint);
PCCX_API int pccx_fps_coop(const float *xyz, int B, int N, int npoint, const int32_t *start_idx, int64_t *idx_out, int G,
                           void *workspace, void *stream);

/* Block-parallel centre selection: P independent farthest point samplings per cloud, side by side (one launch of P * B workgroups of
 * 1024 threads; no cooperative launch, no workspace, no read-back, so it can be captured).  NOT the indices of pccx_fps unless P == 1.
 * order: (B,N) int64, a permutation of 0..N-1 per cloud (in use: the cloud's Morton order); checked for range only -- an entry
 * outside 0..N-1 is clamped and never forms an address.  Block j = 0..P-1 of a cloud holds the sorted positions [lo_j, lo_{j+1}),
 * lo_j = floor(j*N/P) (64-bit), and fills the output slots [o_j, o_{j+1}), o_j = floor(j*npoint/P); its local point i is
 * xyz[order[lo_j + i]], its first centre the local index start_idx[b] mod n_j (0 when start_idx is NULL or the entry lies outside
 * 0..N-1).  Inside a block the recurrence is pccx_fps's to the operation (running minimum from 1e10, (dx*dx + dy*dy) + dz*dz without
 * contraction, fminf, the largest minimum, ties to the LOWER LOCAL index); slot o_j + t receives order[lo_j + winner_t], an index
 * into the original cloud.  PCCX_ERR_ARG before any launch: P < 1, ceil(N/P) > 16384 (a block lives in one workgroup's registers),
 * floor(npoint/P) < 1, ceil(npoint/P) > floor(N/P). */
PCCX_API int pccx_fps_blocks(const float *xyz, int B, int N, const int64_t *order, int P, int npoint, const int32_t *start_idx,
                             int64_t *idx_out, void *stream);

/* 63-bit Morton keys over the bounding box [lo, lo+extent]^3 (lo_host: 3 floats on the HOST), used to
 * cut clouds larger than one block into spatially compact 8192-point blocks (BASELINE configs[3]).
 * xyz: (n,3) f32; keys: (n) int64. */
PCCX_API int pccx_morton_keys(const float *xyz, int64_t n, const float *lo_host, float extent, int64_t *keys,
                              void *stream);
/* The same keys over the cloud's own bounding box, found on the device (bbox_workspace: 6 int32 on the device, scratch): no
 * host round trip, so the block partition of a large cloud can be queued without a synchronisation. */
PCCX_API int pccx_morton_keys_auto(const float *xyz, int64_t n, int64_t *keys, int32_t *bbox_workspace, void *stream);

/* The block partition of a room-scale cloud (BASELINE configs[3]; the reference has no such path: octree_np.decode hard-codes S = 64,
 * octree_np.py:100, so a cloud of N points is cut into blocks of 8192).  pccx_sort_keys_u64: STABLE ascending radix sort of the keys IN
 * PLACE; order (n) int64 = the input position of the key at each sorted position (torch.sort(keys, stable=True).indices).  key_bits:
 * significant low bits (63 for the Morton keys).  workspace: pccx_sort_keys_workspace_bytes(n) bytes, 16-byte aligned; n < 2^32. */
PCCX_API size_t pccx_sort_keys_workspace_bytes(int64_t n);
PCCX_API int pccx_sort_keys_u64(int64_t *keys, int64_t n, int key_bits, int64_t *order, void *workspace, void *stream);
/* blocks_out (count, block, 3): block b = rows order[(first + b * stride) * block + i], i < block, of pc (n,3); positions >= n repeat
 * row order[n - 1] (the last block is completed with copies of its final point).  first / stride select a rank's blocks. */
PCCX_API int pccx_gather_blocks(const float *pc, const int64_t *order, int64_t n, int block, int64_t first, int64_t stride,
                                int64_t count, float *blocks_out, void *stream);
/* The inverse: pc_out[order[(first + b * stride) * block + i]] = rows_in[b][i] for every position < n (padding rows are dropped). */
PCCX_API int pccx_scatter_blocks(const float *rows_in, const int64_t *order, int64_t n, int block, int64_t first, int64_t stride,
                                 int64_t count, float *pc_out, void *stream);

/* pn_kit.index_points (pn_kit.py:332-360) / pytorch3d knn_gather (pointnet_sa_module.py:28):
 * out[b,m,:] = points[b, idx[b,m], :].  points: (B,N,C); idx: (B,M) int64 (negative -> row 0,
 * the clamp of pointnet_sa_module.py:27); out: (B,M,C). */
PCCX_API int pccx_gather(const float *points, int B, int N, int C, const int64_t *idx, int M,
                         float *out, void *stream);

/* pytorch3d knn_points(p1=q, p2=ref, K, return_nn) (compress.py:71, pn_kit.py:190, eval.py:132):
 * squared L2, K smallest ascending, ties by lower index.  q: (B,M,3); ref: (B,N,3);
 * dists: (B,M,K) f32 or NULL; idx: (B,M,K) int64 or NULL; nn: (B,M,K,3) or NULL (at least one of the three).  K <= 1024, K <= N <= 32768.
 * If patch_scale != 0, nn instead receives (ref[idx]-q)*patch_scale: the fused form of
 * compress.py:72 (subtract centre) and compress.py:108 (scale by (N/N0)^(1/3)). */
PCCX_API int pccx_knn(const float *q, int B, int M, const float *ref, int N, int K, float *dists,
                      int64_t *idx, float *nn, float patch_scale, void *stream);

/* pytorch3d ball_query(p1=q, p2=ref, K, radius) (pointnet_sa_module.py:18): first K indices in
 * index order with d2 < radius^2, padded with -1 (dists padded with 0). */
PCCX_API int pccx_ball_query(const float *q, int B, int M, const float *ref, int N, int K,
                             float radius, float *dists, int64_t *idx, void *stream);
/* The same query through a uniform grid hash of the candidates (cells of side >= radius, 27-cell walk, index order restored by
 * a bitmap): identical results, for large N / small radius.  workspace: pccx_ball_query_grid_workspace_ints(B, N) int32; N <= 32768. */
PCCX_API size_t pccx_ball_query_grid_workspace_ints(int B, int N);
PCCX_API int pccx_ball_query_grid(const float *q, int B, int M, const float *ref, int N, int K, float radius,
                                  int32_t *workspace, float *dists, int64_t *idx, void *stream);

/* One-directional nearest neighbour: for each x in X (B,P,3) the min over Y (B,Q,3) of |x-y|^2.
 * d2: (B,P); nn: (B,P) int32 or NULL.  Building block of pytorch3d chamfer_distance (AE.py:67,
 * eval.py:204) and of eval.py's D1 loop (eval.py:73-81). */
PCCX_API int pccx_nn_dist(const float *X, int B, int P, const float *Y, int Q, float *d2, int32_t *nn,
                          void *stream);
/* pccx_nn_dist for batches too small to fill the chip (configs[4]: 4 clouds): the reference cloud is scanned in `split` chunks by
 * different workgroups (partials in scratch_d / scratch_nn: split * B * P entries each; scratch_nn may be NULL when nn is) and merged
 * by a second kernel; identical results.  pccx_nn_dist_split_count: the split this shape should use (1 = call pccx_nn_dist). */
PCCX_API int pccx_nn_dist_split_count(int B, int P, int Q);
PCCX_API int pccx_nn_dist_split(const float *X, int B, int P, const float *Y, int Q, int split, float *scratch_d, int32_t *scratch_nn,
                                float *d2, int32_t *nn, void *stream);
/* pccx_nn_dist over a ragged batch, the building block of pytorch3d chamfer_distance(x, y, x_lengths=, y_lengths=): X (B,P_max,3),
 * Y (B,Q_max,3); p, q: (B) int32 ON THE DEVICE (a captured step may change them between replays), clamped into [0, P_max] /
 * [0, Q_max] where they are read.  Cloud b queries its first p[b] rows against the first q[b] rows of Y; the rows behind the counts
 * are never loaded (they may hold NaN), d2 / nn (B,P_max) behind p[b] stay unwritten, and the first p[b] entries are bit for bit
 * pccx_nn_dist's on the unpadded pair.  A cloud with a zero count writes nothing. */
PCCX_API int pccx_nn_dist_n(const float *X, int B, int P_max, const int32_t *p, const float *Y, int Q_max, const int32_t *q, float *d2,
                            int32_t *nn, void *stream);

/* Exact nearest-neighbour search through a uniform grid index, for whole rooms (10^5 .. 10^6 points) where the all-pairs kernels
 * above cost P * Q pairs: what open3d's KDTreeFlann.search_knn_vector_3d answers in eval.py:55-81 (30-NN for the normals, 1-NN for
 * D1 / D2) and pytorch3d.ops.knn_points in eval.py:132.  Results are bit for bit those of pccx_nn_dist / pccx_knn: same fp32
 * distance expression, ties to the lower index (csrc/grid_nn.hip carries the argument).
 * pccx_grid_dims: the grid a cloud of N points with bounding-box extents (ex, ey, ez) gets -- dims[3] cells per axis and the cubic
 * cell's side; host only, a pure function (about 2 points per cell of the box, at most 2^21 cells and 1024 per axis; an axis of no
 * extent has one cell).  pccx_grid_index_workspace_bytes / pccx_grid_query_workspace_bytes: host only; 0 for an empty batch.
 * pccx_grid_index_build: the index of Y (B,N,3) into `workspace` (16-byte aligned, kept by the caller for as long as the index is
 * queried; Y itself is not read again): bounding box and grid per cloud on the device, pccx_sort_keys_u64 over (cloud, cell) keys,
 * the points in that order and a cell-start table.  B <= 65535, B * N < 2^31. */
PCCX_API int pccx_grid_dims(int N, float ex, float ey, float ez, int32_t *dims, float *cell);
PCCX_API size_t pccx_grid_index_workspace_bytes(int B, int N);
PCCX_API size_t pccx_grid_query_workspace_bytes(int B, int M);
PCCX_API int pccx_grid_index_build(const float *Y, int B, int N, void *workspace, void *stream);
/* The same index with about `target` >= 2 points per cell instead of 2 (same workspace size, queried by the same entries with the same
 * results): coarser cells for pccx_grid_knn_wide, whose K neighbours span hundreds of the default cells. */
PCCX_API int pccx_grid_index_build_target(const float *Y, int B, int N, int target, void *workspace, void *stream);
/* pccx_nn_dist(X, Y) through the index of Y (B,Q,3): d2 (B,P) f32, nn (B,P) int32 or NULL.  query_workspace:
 * pccx_grid_query_workspace_bytes(B, P) bytes of scratch, 16-byte aligned.  Stands in for the KD-tree's 1-NN of eval.py:73-81. */
PCCX_API int pccx_grid_nn(const float *X, int B, int P, int Q, const void *index, void *query_workspace, float *d2, int32_t *nn,
                          void *stream);
/* pccx_knn(q, ref) through the index of ref (B,N,3), 1 <= K <= min(N, 32): dists (B,M,K) f32 and idx (B,M,K) int64, ascending by
 * (distance, index).  Stands in for search_knn_vector_3d(knn=30) of eval.py:59-60 and knn_points of eval.py:132 at room size. */
PCCX_API int pccx_grid_knn(const float *q, int B, int M, int N, int K, const void *index, void *query_workspace, float *dists,
                           int64_t *idx, void *stream);
/* pccx_knn_list(q, ref) through the index of ref (B,N,3) for the wide K of the codec's patch search, 1 <= K <= min(N, 1024)
 * (KNN_Patching, compress.py:70-74, and the patches of compress.py:105-108): what lets a cloud past pccx_knn's 32768 points be cut into
 * patches as ONE cloud.  One workgroup per query keeps its candidates in LDS.  dists (B,M,K) f32, idx (B,M,K) int64 and nn (B,M,K,3)
 * are each optional (at least one); nn holds ref[idx], or (ref[idx] - q) * patch_scale when patch_scale != 0, read from the index's
 * own copy of the points.  rep: NULL or the (B * M) table of pccx_patch_groups over the queries -- only queries with rep[p] == p are
 * searched, the rows of the others stay unwritten.  Results are bit for bit those of pccx_knn, ascending by (distance bits, index).
 * query_workspace: pccx_grid_knn_wide_workspace_bytes(B, N) bytes (N: the points per cloud of the INDEX), 16-byte aligned; host only,
 * 0 for an empty batch.  K <= 32 is served too (pccx_grid_knn, one wave per query, is the faster kernel there but has no nn and no
 * rep).  B <= 65535, B * M and B * N < 2^31. */
PCCX_API size_t pccx_grid_knn_wide_workspace_bytes(int B, int N);
PCCX_API int pccx_grid_knn_wide(const float *q, int B, int M, int N, int K, const void *index, void *query_workspace, float *dists,
                                int64_t *idx, float *nn, float patch_scale, const int32_t *rep, void *stream);

/* chamfer_distance's value from the two pccx_nn_dist passes dxy (B,P), dyx (B,Q) (pytorch3d defaults: point and batch mean, both
 * directions summed; AE.py:67): out[0] = batch mean of (mean_p dxy + mean_q dyx), accumulated in double */
PCCX_API int pccx_chamfer_mean(const float *dxy, const float *dyx, int B, int P, int Q, float *out, void *stream);
/* Backward of chamfer_distance (batch mean of both directions' point means; AE.py:57-70,
 * pppe_pcd_ae.py:817-838) for fixed argmins nn_xy (B,P), nn_yx (B,Q) from pccx_nn_dist:
 * gX (B,P,3), gY (B,Q,3) receive grad_out * dL/dX, dL/dY (buffers are zeroed here). */
PCCX_API int pccx_chamfer_grad(const float *X, int B, int P, const float *Y, int Q, const int32_t *nn_xy,
                               const int32_t *nn_yx, float grad_out, float *gX, float *gY, void *stream);
/* pccx_chamfer_grad with the upstream gradient scalar read from device memory (no host sync: usable under hipGraph capture). */
PCCX_API int pccx_chamfer_grad_dev(const float *X, int B, int P, const float *Y, int Q, const int32_t *nn_xy,
                                   const int32_t *nn_yx, const float *grad_out_dev, float *gX, float *gY, void *stream);
/* ... into gX / gY the caller cleared (flags & 4) */
PCCX_API int pccx_chamfer_grad_dev_acc(const float *X, int B, int P, const float *Y, int Q, const int32_t *nn_xy,
                                       const int32_t *nn_yx, const float *grad_out_dev, float *gX, float *gY, int flags,
                                       void *stream);
/* The same two for ragged batches: pytorch3d.loss.chamfer_distance's x_lengths / y_lengths (chamfer.py: "Optional LongTensor of shape
 * (N,) giving the number of points in each cloud"), here p, q (B) int32 on the device, as pccx_nn_dist_n takes them.
 * pccx_chamfer_mean_n: out[0] = (1/B) sum_b [ (1/p_b) sum_{i<p_b} dxy[b,i] + (1/q_b) sum_{j<q_b} dyx[b,j] ] in double; dxy (B,P_max),
 * dyx (B,Q_max) from pccx_nn_dist_n; per_cloud: NULL or (B) f32, the bracket of each cloud (batch_reduction=None).  A zero count
 * divides by 1, pytorch3d's clamp.  One launch.
 * pccx_chamfer_grad_n: its backward for the argmins of pccx_nn_dist_n, wx_b = g / (B p_b), wy_b = g / (B q_b), g read from
 * grad_out_dev.  gX (B,P_max,3), gY (B,Q_max,3): cleared here, or accumulated into when flags & 4 says the caller cleared them; rows
 * >= p[b] of gX and >= q[b] of gY end as exact zeros.  Atomic scatter, as pccx_chamfer_grad: there is no deterministic form. */
PCCX_API int pccx_chamfer_mean_n(const float *dxy, const float *dyx, int B, int P_max, const int32_t *p, int Q_max, const int32_t *q,
                                 float *out, float *per_cloud, void *stream);
PCCX_API int pccx_chamfer_grad_n(const float *X, int B, int P_max, const int32_t *p, const float *Y, int Q_max, const int32_t *q,
                                 const int32_t *nn_xy, const int32_t *nn_yx, const float *grad_out_dev, float *gX, float *gY, int flags,
                                 void *stream);

/* D2 (point-to-plane) PSNR support (eval.py:58-60,73-81).  pccx_estimate_normals: PCA normal of
 * every point over its K neighbours nbr (B,N,K) int64 (e.g. pccx_knn with K=30, as open3d's
 * estimate_normals(KDTreeSearchParamKNN(knn=30))); unoriented.  pccx_point_plane_err:
 * err[b,i] = ((X[b,i] - Y[b,nn[b,i]]) . normals_Y[b,nn[b,i]])^2. */
PCCX_API int pccx_estimate_normals(const float *xyz, int B, int N, const int64_t *nbr, int K, float *normals,
                                   void *stream);
PCCX_API int pccx_point_plane_err(const float *X, int B, int P, const float *Y, const float *normals_Y, int Q,
                                  const int32_t *nn, float *err, void *stream);

/* ---- integer path: octree of the S sampled centres ------------------------------------------- */

/* Bytes needed per cloud for the bit array (one byte per bit) of pccx_octree_encode. */
PCCX_API int pccx_octree_bits_capacity(int S);

/* pn_kit.encode_sampled_np (pn_kit.py:380-401) = depth search over octree_np.encode
 * (octree_np.py:10-45) + octree_np.getDecodeFromPc (octree_np.py:114-133), scale = 1, followed by
 * pn_kit.binary_array_to_byte_array (pn_kit.py:463-467).
 * centres: (B,S,3) f32, S <= 1024; N: points per cloud (bpp denominator); min_bpp as
 * pn_kit.OCTREE_BPP_DICT[K].
 * bits:   (B,cap) uint8, one byte per bit, cap = pccx_octree_bits_capacity(S);
 * nbits:  (B) int32 stream length in bits;  depth: (B) int32 (DEPTH as the reference leaves it);
 * bytes:  (B,(cap+7)/8) uint8 packed stream, last partial byte right-aligned; nbytes: (B) int32. */
PCCX_API int pccx_octree_encode(const float *centres, int B, int S, int N, double min_bpp,
                                uint8_t *bits, int32_t *nbits, int32_t *depth, uint8_t *bytes,
                                int32_t *nbytes, void *stream);
/* The same outputs, bit for bit, for 1 <= S <= 8192 centres: 1024 threads with up to 8 sorted keys each (the sort runs over up to
 * 8192 keys in 64 KB of LDS).  pccx_octree_encode keeps its own kernel and its limit. */
PCCX_API int pccx_octree_encode_wide(const float *centres, int B, int S, int N, double min_bpp,
                                     uint8_t *bits, int32_t *nbits, int32_t *depth, uint8_t *bytes,
                                     int32_t *nbytes, void *stream);

/* pn_kit.decode_sampled_np -> octree_np.decode (octree_np.py:47-112) from the packed stream
 * (decompress.py:80-83 unpacks with pn_kit.byte_array_to_binary_array first).
 * mode 0 = "reference": bug-compatible with octree_np.decode as written (only the first 8 bits are
 *          consumed; output padded to 64 points);  S_out must be 64.
 * mode 1 = "full": level-by-level decode (the build's extension), descending-Morton order; the
 *          first min(count,S_out) points are written, the rest repeat the last point.
 * bytes: (B,stride) uint8; nbytes: (B) int32; out: (B,S_out,3) f32; count: (B) int32 decoded points.
 *
 * Streams nobody encoded.  Every byte string decodes to something defined or is refused; nothing past a row is read or written.
 * nbytes is clamped to [0, stride] (mode 0 only tells "<= 0" from the rest: it reads byte 0 alone).
 * mode 0: nbytes <= 0 gives the single point (0.5,0.5,0.5), count 1.  Otherwise the eight bits of byte 0, MSB first, are the children
 *   111..000 of the root: count = popcount(byte 0) points in {0.25,0.75}^3, padded to 64 with the last one, all zeros when count = 0.
 *   This is octree_np.decode of byte_array_to_binary_array(bytes) for all 256 values of byte 0, whatever follows it.
 * mode 1: the stream is the 8*(nbytes-1) + 1 bits the encoder packs: nbytes-1 whole bytes MSB first, then ONE bit, the lowest bit of
 *   the last byte (pn_kit.py:465-466 right-aligns a final partial group; the other seven bits of that byte are not read, so a stream
 *   cut at a byte boundary reads its last byte as that one bit).  Bit 0 is the root; level l+1 is the next 8*popcount(level l) bits
 *   and is taken only when all of them are inside the stream, so trailing bits that do not fill a level are ignored.  An empty
 *   stream, a root bit of 0 or an all-zero level give count 0 and out = 0.  Otherwise count = popcount of the last level taken, and
 *   min(count,S_out) leaves are written followed by copies of the last one; S_out < count writes the first S_out only.
 *   count = -1 refuses the stream and leaves its out row untouched: a level of more than 2048 occupied cells, or a whole level
 *   present below level 16 (the encoder never writes either: S <= 1024 and DEPTH <= 16).  A deeper stream is NOT cut at level 16.
 *   With S_out > 1024 the wide kernel decodes (1024 threads, 8192 codes per level in 128 KB of LDS): the same rules with the refusal
 *   at a level of more than 8192 occupied cells, for the streams of pccx_octree_encode_wide.
 * mode 2 = mode 1 through the wide kernel whatever S_out (the same points and counts wherever mode 1's kernel accepts the stream). */
PCCX_API int pccx_octree_decode(const uint8_t *bytes, int stride, const int32_t *nbytes, int B,
                                int mode, int S_out, float *out, int32_t *count, void *stream);

/* ---- neural transforms (fp32 on the matrix cores) --------------------------------------------- */

/* Packed weight blobs.  pccx_pack_* run on the HOST, once per model load: every pointer they take
 * is a HOST pointer to a dense row-major fp32 tensor with the shape of the reference's state_dict
 * entry named in the comment; the caller uploads the resulting blob.
 * Limits: bottleneck d <= 16, d*L <= 128; layer widths are those of AE.py. */
PCCX_API size_t pccx_ae_encoder_blob_floats(void);
/* AE.AE.sa / AE.AE.pn (AE.py:16-17): sa.conv0 (32,3) sa.conv1 (64,32) sa.conv2 (128,64)
 * pn.mlp_Modules.{0,1,2,3}.0 (128,131) (256,128) (512,256) (d,512), each with its bias. */
PCCX_API int pccx_pack_ae_encoder(const float *sa_w0, const float *sa_b0, const float *sa_w1,
                                  const float *sa_b1, const float *sa_w2, const float *sa_b2,
                                  const float *pn_w0, const float *pn_b0, const float *pn_w1,
                                  const float *pn_b1, const float *pn_w2, const float *pn_b2,
                                  const float *pn_w3, const float *pn_b3, int d, float *blob_host);
PCCX_API size_t pccx_ae_decoder_blob_floats(int k);
/* AE.AE.inv_pool / inv_mlp (AE.py:19-27): inv_pool.{0,2,4} (256,d) (1024,256) (k*128,1024);
 * inv_mlp.mlp_Modules.{0,1,2,3}.0 (128,128+d) (64,128) (32,64) (3,32). */
PCCX_API int pccx_pack_ae_decoder(const float *ip_w0, const float *ip_b0, const float *ip_w1,
                                  const float *ip_b1, const float *ip_w2, const float *ip_b2,
                                  const float *m_w0, const float *m_b0, const float *m_w1,
                                  const float *m_b1, const float *m_w2, const float *m_b2,
                                  const float *m_w3, const float *m_b3, int k, int d, float *blob_host);
PCCX_API size_t pccx_prob_blob_floats(void);
/* AE.ConditionalProbabilityModel (AE.py:96-105): model_pn.mlp_Modules.{0,1,2}.0 (64,3) (128,64)
 * (256,128); model_mlp.{0,2,4} (512,259) (512,512) (d*L,512). */
PCCX_API int pccx_pack_prob(const float *p_w0, const float *p_b0, const float *p_w1, const float *p_b1,
                            const float *p_w2, const float *p_b2, const float *m_w0, const float *m_b0,
                            const float *m_w1, const float *m_b1, const float *m_w2, const float *m_b2,
                            int d, int L, float *blob_host);

/* Analysis transform of AE.AE.forward (AE.py:37-45) = the two per-patch loops of
 * compress.py:113-127: ae.sa (pn_kit.py:164-211), ae.pn (pn_kit.py:124-144), sigmoid spread, round.
 * patches: (P,K,3) f32, already centred and scaled (compress.py:105-108); K % 16 == 0, K <= 1024.
 * feat_ws: workspace of P*K*128 floats.  Outputs (P,d) f32: latent_raw (PointNet output),
 * latent (after sigmoid spread), latent_q (rounded).  Spread is L - 0.2. */
PCCX_API int pccx_ae_encode(const float *patches, int P, int K, const float *enc_blob, int d, int L,
                            float *feat_ws, float *latent_raw, float *latent, float *latent_q,
                            void *stream);

/* The two halves of pccx_ae_encode, as the reference calls them (compress.py:114 ae.sa,
 * compress.py:121 ae.pn).  feat: (P,8,K,16) f32 = the (P,128,K) SetAbstraction feature map with
 * channels grouped by 16 (feat[p][c/16][i][c%16]), the layout pccx_pn_forward consumes. */
PCCX_API int pccx_sa_forward(const float *patches, int P, int K, const float *enc_blob, float *feat,
                             void *stream);
PCCX_API int pccx_pn_forward(const float *patches, const float *feat, int P, int K,
                             const float *enc_blob, int d, int L, float *latent_raw, float *latent,
                             float *latent_q, void *stream);

PCCX_API size_t pccx_ae_decode_workspace_floats(int P);
/* Synthesis transform (AE.py:48-53 = decompress.py:97-102) and, optionally, the reassembly of
 * decompress.py:104-116.  latent_q: (P,d) f32; workspace: pccx_ae_decode_workspace_floats(P).
 * patches_out (P,k,3) or NULL: raw decoder output (new_xyz.transpose(2,1)).
 * pc_out (P*k,3) or NULL: ((patch / scale) + centres[patch] - 0.5) * longest[b] / (1-margin) +
 * center[b] with b = patch / S; needs centres (P,3), nrm_center (B,3), nrm_longest (B). */
PCCX_API int pccx_ae_decode(const float *latent_q, int P, int d, int k, const float *dec_blob,
                            float *workspace, float *patches_out, float scale, const float *centres,
                            const float *nrm_center, const float *nrm_longest, int S, double margin,
                            float *pc_out, void *stream);

/* The bf16x3 arithmetic mode (the default of the host layer since round 2, validated against every
 * oracle / golden parity test at the f32 tolerances): the same synthesis transform with the K = 1024 Linear and inv_mlp evaluated as
 * fp32 products of three bf16 pieces per operand on the bf16 matrix cores (six v_mfma_f32_16x16x32_bf16 passes,
 * fp32 accumulate; error at the level of an fp32 summation reorder, not bit-identical to pccx_ae_decode).
 * b3_blob: pccx_dec_b3_blob_floats(k) floats on the device, filled once from the packed decoder blob (already on
 * the device) by pccx_pack_ae_decoder_b3.  workspace: pccx_ae_decode_b3_workspace_floats(P).  Replaces the same
 * reference lines as pccx_ae_decode (AE.py:48-53, decompress.py:97-116). */
PCCX_API size_t pccx_sa_b3_blob_floats(void);
PCCX_API int pccx_pack_sa_b3(const float *enc_blob_dev, float *sa_b3_blob_dev, void *stream);
/* pccx_sa_forward (pn_kit.py:164-211) with conv1 / conv2 on bf16x3 operands. */
PCCX_API int pccx_sa_forward_b3(const float *patches, int P, int K, const float *enc_blob, const float *sa_b3_blob,
                                float *feat, void *stream);
PCCX_API size_t pccx_pn_b3_blob_floats(void);
PCCX_API int pccx_pack_pn_b3(const float *enc_blob_dev, float *pn_b3_blob_dev, void *stream);
/* pccx_pn_forward (pn_kit.py:124-144, AE.py:43-45) on bf16x3 operands. */
PCCX_API int pccx_pn_forward_b3(const float *patches, const float *feat, int P, int K, const float *enc_blob,
                                const float *pn_b3_blob, int d, int L, float *latent_raw, float *latent,
                                float *latent_q, void *stream);
/* pccx_sa_forward_b3 + pccx_pn_forward_b3 in ONE kernel (compress.py:113-127: ae.sa, ae.pn, sigmoid spread, round): the
 * (P,128,K) feature map of ae.sa stays inside the CU instead of making a round trip through HBM.  Same blobs, same arithmetic
 * and results as the two calls.  pccx_ae_encode_b3_fused_ok(K) tells whether a K-point patch fits the kernel's LDS budget
 * (K <= 512); otherwise run the two calls through a feature workspace. */
PCCX_API int pccx_ae_encode_b3_fused_ok(int K);
PCCX_API int pccx_ae_encode_b3(const float *patches, int P, int K, const float *enc_blob, const float *sa_b3_blob,
                               const float *pn_b3_blob, int d, int L, float *latent_raw, float *latent,
                               float *latent_q, void *stream);
/* The in-patch neighbour selection SetAbstraction starts with (pn_kit.py:186-190: knn_points(xyz, xyz, K=16) on each
 * (K,3) patch) as a kernel of its own: pure vector-ALU work that runs at 8 waves per SIMD here instead of the encoder's 2.
 * Table layout nbr[P][K][16], pccx_patch_knn16_index_bytes(K) bytes per index (1 while K <= 256, else 2), 16-byte aligned,
 * pccx_patch_knn16_bytes(P, K) bytes in all.  Rows hold the SET of the 16 nearest points under the oracle's (distance, index)
 * order (orc_knn); the order inside a row is unspecified (a max-pool follows, pn_kit.py:211). */
PCCX_API int pccx_patch_knn16_index_bytes(int K);
PCCX_API size_t pccx_patch_knn16_bytes(int P, int K);
PCCX_API int pccx_patch_knn16(const float *patches, int P, int K, void *nbr, void *stream);
/* pccx_ae_encode_b3 with the neighbour selection taken out into pccx_patch_knn16 (both launched from this call): the form
 * the host layer uses.  workspace: pccx_ae_encode_b3_workspace_bytes(P, K) bytes on the device, 16-byte aligned.  Results are
 * bit-identical to pccx_ae_encode_b3. */
PCCX_API size_t pccx_ae_encode_b3_workspace_bytes(int P, int K);
PCCX_API int pccx_ae_encode_b3_ws(const float *patches, int P, int K, const float *enc_blob, const float *sa_b3_blob,
                                  const float *pn_b3_blob, int d, int L, float *latent_raw, float *latent,
                                  float *latent_q, void *workspace, void *stream);
/* The fused kernel of pccx_ae_encode_b3_ws ALONE, on neighbour tables the caller has filled with pccx_patch_knn16(patches, P, K,
 * tables, stream): the two launches as two calls, for a host that times or schedules them separately (bench.py's stage table).
 * Replaces the same lines (compress.py:113-127). */
PCCX_API int pccx_ae_encode_b3_tables(const float *patches, int P, int K, const float *enc_blob, const float *sa_b3_blob,
                                      const float *pn_b3_blob, int d, int L, float *latent_raw, float *latent,
                                      float *latent_q, const void *tables, void *stream);
PCCX_API size_t pccx_dec_b3_blob_floats(int k);
PCCX_API int pccx_pack_ae_decoder_b3(const float *dec_blob_dev, int k, float *b3_blob_dev, void *stream);
PCCX_API size_t pccx_ae_decode_b3_workspace_floats(int P);
PCCX_API int pccx_ae_decode_b3(const float *latent_q, int P, int d, int k, const float *dec_blob,
                               const float *b3_blob, float *workspace, float *patches_out, float scale,
                               const float *centres, const float *nrm_center, const float *nrm_longest,
                               int S, double margin, float *pc_out, void *stream);

/* The f16x2 arithmetic mode: the same two transforms with every fp32 product formed from TWO fp16 pieces
 * per operand (hi = rn16(x), lo = rn16(x - hi): 22-23 significant bits, the operand precision of "3xTF32") and three
 * v_mfma_f32_16x16x32_f16 passes, fp32 accumulate -- half the matrix instructions of bf16x3.  fp16's narrow exponent is handled by
 * exact power-of-two scales: static ones per layer from rigorous interval bounds of the layers (computed when the weights are
 * packed) and one per patch from the data (largest |coordinate| / head activation), so no operand can overflow and the lo piece
 * keeps its bits; powers of two commute with fp32 rounding, so the scaled chain computes what the unscaled one would.
 * The blobs are built on the HOST from the same state_dict tensors as pccx_pack_ae_encoder / pccx_pack_ae_decoder (HOST pointers,
 * same argument order) and uploaded by the caller.
 * pccx_ae_encode_h2_ws replaces compress.py:113-127 (ae.sa, ae.pn, sigmoid spread, round) like pccx_ae_encode_b3_ws; enc_blob is
 * the fp32 blob (conv0 of SetAbstraction stays an fp32 MFMA), workspace holds the neighbour tables of pccx_patch_knn16.
 * pccx_ae_decode_h2 replaces AE.py:48-53 / decompress.py:97-116 like pccx_ae_decode_b3; dec_blob is the fp32 blob (the two head
 * Linears stay fp32 MFMAs). */
PCCX_API size_t pccx_ae_encoder_h2_blob_floats(void);
PCCX_API int pccx_pack_ae_encoder_h2(const float *sa_w0, const float *sa_b0, const float *sa_w1, const float *sa_b1,
                                     const float *sa_w2, const float *sa_b2, const float *pn_w0, const float *pn_b0,
                                     const float *pn_w1, const float *pn_b1, const float *pn_w2, const float *pn_b2,
                                     const float *pn_w3, const float *pn_b3, int d, float *h2_blob);
PCCX_API int pccx_ae_encode_h2_fused_ok(int K);
PCCX_API size_t pccx_ae_encode_h2_workspace_bytes(int P, int K);
PCCX_API int pccx_ae_encode_h2_ws(const float *patches, int P, int K, const float *enc_blob, const float *h2_blob, int d, int L,
                                  float *latent_raw, float *latent, float *latent_q, void *workspace, void *stream);
/* the fused f16x2 kernel alone on caller-filled tables, as pccx_ae_encode_b3_tables (compress.py:113-127) */
PCCX_API int pccx_ae_encode_h2_tables(const float *patches, int P, int K, const float *enc_blob, const float *h2_blob, int d, int L,
                                      float *latent_raw, float *latent, float *latent_q, const void *tables, void *stream);
PCCX_API size_t pccx_ae_decoder_h2_blob_floats(int k);
PCCX_API int pccx_pack_ae_decoder_h2(const float *ip_w0, const float *ip_b0, const float *ip_w1, const float *ip_b1,
                                     const float *ip_w2, const float *ip_b2, const float *m_w0, const float *m_b0,
                                     const float *m_w1, const float *m_b1, const float *m_w2, const float *m_b2,
                                     const float *m_w3, const float *m_b3, int k, int d, float *h2_blob);
PCCX_API size_t pccx_ae_decode_h2_workspace_floats(int P);
PCCX_API int pccx_ae_decode_h2(const float *latent_q, int P, int d, int k, const float *dec_blob, const float *h2_blob,
                               float *workspace, float *patches_out, float scale, const float *centres,
                               const float *nrm_center, const float *nrm_longest, int S, double margin, float *pc_out,
                               void *stream);

/* ---- duplicate patches (csrc/patch_groups.hip) ---------------------------------------------------------------------------
 * In octree_mode "reference" a cloud has at most 8 distinct patch centres (the bug-compatible decode reads one byte of the
 * stream; rows np-1 .. 63 repeat the last centre), so most of a batch's patches are copies of an earlier patch of their cloud.
 * pccx_patch_groups finds them on the device: key row of patch p = floats_a words of keys_a row p followed by floats_b words of
 * keys_b row p (keys_b may be NULL with floats_b = 0), compared as uint32 words.  rep (B*S) int32: the smallest patch of p's cloud
 * with an equal key row (rep[p] == p: a representative); uniq (B*S) int32: the representatives in ascending order; n_uniq: their
 * count, 1 int32 ON THE DEVICE -- nothing returns to the host.  workspace: pccx_patch_groups_workspace_ints(B) int32.  1 <= S <= 1024.
 * The *_list entry points below take uniq / n_uniq (or rep), do the listed patches only and leave the rows of the others as they
 * were; NULL lists mean every patch, bit for bit the entry point without the suffix.  pccx_replicate_rows then overwrites, in up to
 * three (P, row_floats) arrays (a1, a2 may be NULL), every row p with rep[p] != p by row rep[p]. */
PCCX_API size_t pccx_patch_groups_workspace_ints(int B);
PCCX_API int pccx_patch_groups(const float *keys_a, int floats_a, const float *keys_b, int floats_b, int B, int S, int32_t *rep,
                               int32_t *uniq, int32_t *n_uniq, int32_t *workspace, void *stream);
/* The same tables for 1 <= S <= 8192 patches per cloud: an open-addressing table in LDS in place of the all-earlier-rows compare
 * (csrc/patch_groups.hip).  Same arguments and workspace. */
PCCX_API int pccx_patch_groups_wide(const float *keys_a, int floats_a, const float *keys_b, int floats_b, int B, int S, int32_t *rep,
                                    int32_t *uniq, int32_t *n_uniq, int32_t *workspace, void *stream);
PCCX_API int pccx_replicate_rows(const int32_t *rep, int64_t P, int row_floats, float *a0, float *a1, float *a2, void *stream);
/* pccx_knn for the queries with rep[b*M + m] == b*M + m only (rep over the (B, M) queries; NULL = all). */
PCCX_API int pccx_knn_list(const float *q, int B, int M, const float *ref, int N, int K, float *dists, int64_t *idx, float *nn,
                           float patch_scale, const int32_t *rep, void *stream);
/* pccx_knn for the queries uniq[0 .. *n_uniq) only (pccx_patch_groups over the (B, M) queries; both on the device, NULL = all): the
 * workgroups walk the list instead of one being launched per query.  The list form covers the shapes pccx_knn_uniq_ok(N, K) accepts
 * (host only, a pure function: N <= 8192, K <= 256). */
PCCX_API int pccx_knn_uniq_ok(int N, int K);
PCCX_API int pccx_knn_uniq(const float *q, int B, int M, const float *ref, int N, int K, float *dists, int64_t *idx, float *nn,
                           float patch_scale, const int32_t *uniq, const int32_t *n_uniq, void *stream);
PCCX_API int pccx_patch_knn16_list(const float *patches, int P, int K, void *nbr, const int32_t *uniq, const int32_t *n_uniq,
                                   void *stream);
PCCX_API int pccx_ae_encode_h2_tables_list(const float *patches, int P, int K, const float *enc_blob, const float *h2_blob, int d,
                                           int L, float *latent_raw, float *latent, float *latent_q, const void *tables,
                                           const int32_t *uniq, const int32_t *n_uniq, void *stream);
/* The decoder over the listed patches (keys: centre row + latent_q row): each result lands in its own patch's place of patches_out /
 * pc_out; pccx_replicate_rows with row_floats = 3 k fills the places of the copies. */
PCCX_API int pccx_ae_decode_h2_list(const float *latent_q, int P, int d, int k, const float *dec_blob, const float *h2_blob,
                                    float *workspace, float *patches_out, float scale, const float *centres,
                                    const float *nrm_center, const float *nrm_longest, int S, double margin, float *pc_out,
                                    const int32_t *uniq, const int32_t *n_uniq, void *stream);
/* The same for a list much shorter than P (octree_mode "reference"): the head takes one listed tile per workgroup.  Same results. */
PCCX_API int pccx_ae_decode_h2_short_list(const float *latent_q, int P, int d, int k, const float *dec_blob, const float *h2_blob,
                                          float *workspace, float *patches_out, float scale, const float *centres,
                                          const float *nrm_center, const float *nrm_longest, int S, double margin, float *pc_out,
                                          const int32_t *uniq, const int32_t *n_uniq, void *stream);

/* AE.ConditionalProbabilityModel.forward (AE.py:107-123) + pn_kit.pmf_to_cdf (pn_kit.py:452-461)
 * + torchac's float-CDF -> 16-bit conversion.  centres: (B,S,3), S % 16 == 0.  Any of the outputs
 * may be NULL: pmf (B,S,d,L) f32; cdf (B,S,d,L+1) f32; cdf_int (B,S,d,L+1) int32 holding uint16. */
PCCX_API int pccx_prob_forward(const float *centres, int B, int S, int d, int L, const float *prob_blob,
                               float *pmf, float *cdf, int32_t *cdf_int, void *stream);
/* The same outputs, bit for bit, for clouds whose centres repeat (octree_mode "reference": at most 8 distinct rows among 64): each
 * distinct centre row of a cloud (compared bit for bit) is evaluated once and its tables are copied to the duplicates.  S <= 64. */
PCCX_API int pccx_prob_forward_distinct(const float *centres, int B, int S, int d, int L, const float *prob_blob,
                                        float *pmf, float *cdf, int32_t *cdf_int, void *stream);
/* The same outputs, bit for bit, with the 16-centre tiles of every cloud dealt over the chip (opt-in; for few clouds of many centres,
 * a whole room's 8192: pccx_prob_forward gives a cloud to one workgroup).  Three launches in stream order, no cooperative launch:
 * pass 1 on a grid of (min(ceil(S/64), 64), B) workgroups, whose 256 partial maxima each go to workspace; one workgroup per cloud
 * reduces them and runs pass 1b (512 floats per cloud, also in workspace); pass 2 + softmax + the tables on a grid of
 * (ceil(S/64), B), four tiles per workgroup in one pass over the weights.  fmaxf is exact in any grouping and a centre's chain is
 * pccx_prob_forward's k-tile for k-tile, hence the equality.  workspace: pccx_prob_forward_tiled_workspace_floats(B, S) floats on
 * the device (host only; 0 for B < 1 or S < 16), 16-byte aligned, free for reuse once the call's launches have run.  The S / d / L
 * limits are pccx_prob_forward's; B <= 65535 (the grid's second dimension); B = 0 launches nothing. */
PCCX_API size_t pccx_prob_forward_tiled_workspace_floats(int B, int S);
PCCX_API int pccx_prob_forward_tiled(const float *centres, int B, int S, int d, int L, const float *prob_blob,
                                     float *pmf, float *cdf, int32_t *cdf_int, float *workspace, void *stream);

/* torchac.encode_float_cdf (compress.py:134-136) / decode_float_cdf (decompress.py:92-93) on the
 * integer CDFs of pccx_prob_forward.  One independent stream per cloud of nsym = S*d symbols.
 * latent_q: (B,nsym) f32 integer-valued in [-(L/2), L/2]; out: (B,cap) bytes; nbytes: (B) int32
 * (negative = capacity exceeded, |value| bytes were needed).
 *
 * cdf_int rows hold L+1 entries, entry 0 = 0, entry L standing for 2^16 whatever it stores; the coder is defined for rows that give
 * every one of the L symbols a width of at least 1 (entry l+1 > entry l, entry L-1 < 2^16).
 * Encode: the symbol is (int)latent_q + L/2 clamped to [0, L-1].  Row b of out receives the first min(|nbytes[b]|, cap) bytes of the
 *   stream and nothing else: bytes from there to the end of the row keep what they held, and on overflow the cap bytes written are
 *   the prefix of the full stream.
 * Decode: nbytes[b] is clamped to [0, stride], and bits past the stream read as zero, as torchac reads them.  Any byte string
 *   therefore decodes, a truncated or empty one included, to nsym symbols in [0, L-1]: low <= value <= high holds after every
 *   symbol, so no stream is refused and none is "corrupt" to this layer.  Symbol for symbol the result is what the bit-at-a-time
 *   coder gives on the same bytes, and encoding it again yields a stream that decodes to the same symbols.
 * Each direction has two kernels with identical results, chosen by pccx_range_coder_form (0 = one wave per cloud, staged in LDS;
 * 1 = one lane per cloud from global memory): encode takes 0 while nsym*8 + round4(cap) <= 60 KiB, decode while
 * round4(nsym*(L+1)*2) + round4(stride) + nsym <= 60 KiB and 2 <= L <= 63.  The query takes cap for decode = 0, stride otherwise. */
PCCX_API int pccx_range_coder_form(int decode, int nsym, int L, int cap_or_stride);
PCCX_API int pccx_range_encode(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int L,
                               uint8_t *out, int cap, int32_t *nbytes, void *stream);
PCCX_API int pccx_range_decode(const int32_t *cdf_int, const uint8_t *in, int stride,
                               const int32_t *nbytes, int B, int nsym, int L, float *latent_q,
                               void *stream);

/* Split form of the range-coded latent stream (opt-in; NOT a file the reference reads): the nsym symbols of a cloud are cut into
 * P = ceil(nsym / seg_sym) independent segments, each coded by one wave exactly as pccx_range_encode codes a stream of that many
 * symbols (fresh low / high, the same flush, zero-padded last byte), behind a directory of their byte counts.  Little-endian:
 *     "PXS1" | nsym u32 | seg_sym u16 | reserved u16 = 0 | len[P] u16 | the P segment streams in order
 * (nsym = 0: the 12 fixed bytes).  Both entry points always run the wave kernels and refuse, before anything is launched, L outside
 * 2 .. 63, P above 8192, B above 65535 and a seg_sym above pccx_range_split_max_seg_sym(L) (host only: the largest seg_sym whose
 * LDS images, at 2*seg_sym + 16 bytes per segment, fit the wave kernels' 60 KiB in both directions; 0 for an L they do not take).
 * workspace: pccx_range_split_workspace_bytes(B, nsym, seg_sym) bytes on the device (host only; either direction: the encoder's
 * (B*P) counts and (B*P, 2*seg_sym + 16) segment rows, the decoder's (B, P+1) offsets), 16-byte aligned.
 * Encode: two launches (segments, then one pack kernel).  nbytes[b] = the file length, or -(bytes needed) when cap is too small;
 *   row b of out receives the first min(|nbytes[b]|, cap) bytes of the file and nothing else.
 * Decode: nbytes[b] is clamped to [0, stride]; a check kernel writes status[b] (below) and the segment offsets, then every segment is
 *   decoded at its offset with its own length as the stream length (bytes past a segment read as zero).  A cloud whose status is
 *   not 0 decodes every segment as from an empty stream: deterministic, and no byte of it is read beyond the check.
 * pccx_split_stream_check_host: the same check (csrc/split_stream.h, one function for host and device) on host bytes, no GPU call;
 *   segcap = 2*seg_sym + 16.  Returns the status: 0 ok; 1 shorter than its header, or wrong magic; 2 nsym / seg_sym / reserved
 *   disagree with the call; 3 a length above segcap, or header + sum of the lengths != nbytes.  It reads no byte at or after nbytes. */
PCCX_API int pccx_range_split_max_seg_sym(int L);
PCCX_API size_t pccx_range_split_workspace_bytes(int B, int nsym, int seg_sym);
PCCX_API int pccx_split_stream_check_host(const uint8_t *bytes, int64_t nbytes, int nsym, int seg_sym, int segcap);
PCCX_API int pccx_range_encode_split(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int seg_sym, int L,
                                     uint8_t *out, int cap, int32_t *nbytes, void *workspace, void *stream);
PCCX_API int pccx_range_decode_split(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B,
                                     int nsym, int seg_sym, int L, float *latent_q, int32_t *status, void *workspace,
                                     void *stream);

/* ---- region decode: the patches of ONE whole-room cloud that a box needs --------------------------------
 * The reference has nothing like it (it stops at S = 64).  A cloud written with the split stream in segments of G patches is
 * entered at its segments: these four entry points select the patches, evaluate the probability model for the touched segments'
 * rows only, and decode those segments only.  Every result is, bit for bit, the corresponding rows of the full decode.
 *
 * pccx_region_select: one workgroup of 1024 threads, 1 <= S <= 8192, G >= 1.  centres (S,3) decoded patch centres; c4 = the four
 *   floats of .c.bin on the device (centre xyz, longest side); box_host = lo xyz, hi xyz, six finite floats on the HOST with
 *   lo <= hi, in the cloud's original coordinates; halo finite, >= 0.  Patch p is selected iff lo[a] - halo <= w[p][a] <= hi[a] + halo
 *   on the three axes in fp32, w = pccx_denormalize of the centres (the same four rounded steps).  Outputs on the device, ascending,
 *   from a block prefix scan (identical on every run): patch_idx (S) int64, the first n_sel valid; seg_idx (ceil(S/G)) int32, the
 *   touched segments, the first n_seg valid; rows (S) int64, per selected patch (rank of its segment in seg_idx) * G + p % G;
 *   counts (2) int32 = {n_sel, n_seg}.
 * pccx_prob_feature: passes 1 and 1b of pccx_prob_forward for one cloud, S % 16 == 0: the tiles of 16 centres over up to 64
 *   workgroups, whose 256 partial maxima each go to workspace (pccx_prob_feature_workspace_floats(S) floats, host only), then one
 *   workgroup reduces them and writes feature (512 floats, 16-byte aligned).  Two launches in stream order.
 * pccx_prob_rows: pass 2 + softmax + integer CDF of pccx_prob_forward for compact rows: compact row r stands for row
 *   seg_idx[r / G] * G + r % G of the cloud (cut into [0, S - 1]; the rows past S of a ragged last segment are not to be read).
 *   cdf_int (n_seg * G, d, L+1) int32, equal to the same rows of pccx_prob_forward's.  n_seg <= ceil(S/G); the d / L limits are
 *   pccx_prob_forward's.  n_seg = 0 launches nothing.
 * pccx_range_decode_split_list: pccx_range_decode_split for the listed segments of ONE cloud (B = 1; limits and refusals as there).
 *   The check kernel writes status (1) and the offsets into workspace (pccx_range_split_workspace_bytes(1, nsym, seg_sym)); then
 *   wave j decodes segment seg_idx[j] of the file with table rows j*seg_sym ... of cdf_int (n_list*seg_sym, L+1) into rows
 *   j*seg_sym ... of latent_q (n_list*seg_sym); the ragged last segment has nsym - (P-1)*seg_sym symbols.  No byte of an unlisted
 *   segment is read.  n_list = 0 runs the check alone. */
PCCX_API int pccx_region_select(const float *centres, int S, const float *c4, double margin, const float *box_host, float halo, int G,
                                int64_t *patch_idx, int32_t *seg_idx, int64_t *rows, int32_t *counts, void *stream);
PCCX_API size_t pccx_prob_feature_workspace_floats(int S);
PCCX_API int pccx_prob_feature(const float *centres, int S, const float *prob_blob, float *workspace, float *feature, void *stream);
PCCX_API int pccx_prob_rows(const float *centres, int S, int d, int L, const float *prob_blob, const float *feature,
                            const int32_t *seg_idx, int n_seg, int G, int32_t *cdf_int, void *stream);
PCCX_API int pccx_range_decode_split_list(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int nsym,
                                          int seg_sym, int L, const int32_t *seg_idx, int n_list, float *latent_q, int32_t *status,
                                          void *workspace, void *stream);

/* ---- entry-point index of the single stream: parallel and region decode of the reference's own .p.bin ------
 * The stream is pccx_range_encode's, byte for byte.  A sidecar <name>.p.idx holds the coder's state at every seg_sym-th symbol, so
 * that one wave per segment can enter the one stream.  Little-endian (csrc/entry_index.h, one statement for host and device):
 *     "PXI1" | nsym u32 | seg_sym u32 | P u32 | P entries {low u32, high u32, pos u32},  P = ceil(nsym / seg_sym)
 * pos bits 0..30 = the stream bits the decoder has shifted in beyond its first 32 when it reaches symbol p*seg_sym, bit 31 = an
 * underflow run is pending there; the decoder's value is the 32 stream bits at pos with bit 31 inverted under that flag.  Entry 0 is
 * {0, 0xFFFFFFFF, 0}.  pccx_range_index_bytes(nsym, seg_sym) = 16 + 12 P (host only); index rows on the device are that many bytes
 * each and 4-byte aligned.  Limits and refusals are the split path's (L in 2 .. 63, seg_sym <= pccx_range_split_max_seg_sym(L),
 * P <= 8192, B <= 65535), and a stream row of at most 2^27 bytes.
 * pccx_range_encode_indexed: pccx_range_encode (either of its two kernels, the same choice) that also writes row b of index.  The
 *   stream bytes and nbytes are pccx_range_encode's.
 * pccx_range_index_build: the index of existing streams (files the reference wrote): the sequential decoder (either kernel, as
 *   pccx_range_decode chooses) run once, storing its state at every boundary.  latent_q: NULL, or (B,nsym) to receive the symbols too.
 *   Bit for bit the entries the encoder writes for the same stream.
 * pccx_range_decode_indexed: a check kernel writes status[b] and, into workspace (pccx_range_index_workspace_bytes(B, nsym, seg_sym)
 *   bytes, host only), four words per segment; then a P x B grid, one wave per segment, each started from its entry, staging only the
 *   bytes from its position to the next entry's plus the 32-bit window (at most 2*seg_sym + 24).  index (B, idx_stride) bytes;
 *   idx_nbytes: NULL (every row holds idx_stride bytes) or (B) byte counts, clamped to [0, idx_stride].  Status: 0 ok; 1 shorter than
 *   its header, wrong magic, or not 16 + 12 P bytes; 2 nsym / seg_sym / P disagree with the call; 3 a position below the one before;
 *   4 a position beyond 8 * nbytes; 5 consecutive positions more than 8 * (2*seg_sym + 16) bits apart; 6 an entry outside the coder's
 *   post-renormalisation states (low < 2^31 <= high and not (low >= 2^30 and high < 3 * 2^30)), or entry 0 not the initial state.
 *   A cloud whose status is not 0 decodes every segment as an empty stream from the initial state, and no byte of its stream is
 *   read.  A sidecar that passes and is wrong decodes wrong symbols; no address leaves the staged bytes.
 * pccx_range_decode_indexed_list: the same for the listed segments of ONE cloud, as pccx_range_decode_split_list: index = the
 *   idx_bytes bytes of the sidecar, compact table rows and outputs, n_list = 0 runs the check alone.  No byte outside the listed
 *   segments' spans is read.
 * pccx_entry_index_check_host: the same check on host bytes, no GPU call. */
PCCX_API size_t pccx_range_index_bytes(int nsym, int seg_sym);
PCCX_API size_t pccx_range_index_workspace_bytes(int B, int nsym, int seg_sym);
PCCX_API int pccx_entry_index_check_host(const uint8_t *index, int64_t idx_bytes, int64_t stream_bytes, int nsym, int seg_sym);
PCCX_API int pccx_range_encode_indexed(const int32_t *cdf_int, const float *latent_q, int B, int nsym, int seg_sym, int L,
                                       uint8_t *out, int cap, int32_t *nbytes, uint8_t *index, void *stream);
PCCX_API int pccx_range_index_build(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                    int seg_sym, int L, uint8_t *index, float *latent_q, void *stream);
PCCX_API int pccx_range_decode_indexed(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes,
                                       const uint8_t *index, int idx_stride, const int32_t *idx_nbytes, int B, int nsym, int seg_sym,
                                       int L, float *latent_q, int32_t *status, void *workspace, void *stream);
PCCX_API int pccx_range_decode_indexed_list(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes,
                                            const uint8_t *index, int idx_bytes, int nsym, int seg_sym, int L, const int32_t *seg_idx,
                                            int n_list, float *latent_q, int32_t *status, void *workspace, void *stream);
/* The sidecars of B clouds, <dir>/<name>.p.idx, by the host threads of pccx_write_streams_host (names as there).  Write: row b of
 * index_host (B, idx_stride), whole.  Read: the file into row b (a longer file is an error, a shorter one leaves zeros behind it)
 * and its length into idx_nbytes[b]; a missing file is an error. */
PCCX_API int pccx_write_index_host(const void *index_host, int B, int idx_stride, const char *dir, const char *names,
                                   const int64_t *name_off, int threads);
PCCX_API int pccx_read_index_host(void *index_host, int B, int idx_stride, int32_t *idx_nbytes, const char *dir, const char *names,
                                  const int64_t *name_off, int threads);

/* torchac's float -> 16-bit integer CDF conversion (torchac 0.9.3 _convert_to_int_and_normalize with
 * needs_normalization=True, the first step of encode_float_cdf / decode_float_cdf, compress.py:136, decompress.py:93):
 * cdf (nrows, Lp) f32 in [0,1] -> cdf_int (nrows, Lp) int32 holding 16-bit values. */
PCCX_API int pccx_cdf_float_to_int(const float *cdf, int64_t nrows, int Lp, int32_t *cdf_int, void *stream);

/* ---- the three files of every cloud (HOST side; no HIP call) ------------------------------------ */

/* compress.py:139-152 writes <name>.p.bin, <name>.s.bin and <name>.c.bin inside its timer and decompress.py:80-91,113 reads them back
 * inside its own, one Python open/write/close per file.  Here the files of a whole batch are cut from / filled into the HOST copy of the
 * batch's packed stream buffer by `threads` host threads (0 = min(8, hardware threads)).  packed_host: the buffer of
 * pccx_streams_packed_bytes(B, s_stride, p_cap) bytes laid out as
 *     s_nbytes (B) int32 | p_nbytes (B) int32 | c (B,4) f32 [cx,cy,cz,longest] | s_bytes (B,s_stride) u8 | p_bytes (B,p_cap) u8
 * (what the octree / range-coder entry points above write when handed views of one device buffer, copied to the host in one piece).
 * File b is <dir>/<names + name_off[b]><ext> (names: NUL-terminated strings; name_off: (B) int64 offsets into it).  Formats are the
 * reference's: .s.bin = the first s_nbytes[b] bytes of row b, .p.bin = the first p_nbytes[b] bytes of row b, .c.bin = 16 bytes.
 * Write refuses (before touching the file system) a byte count that is negative or exceeds its row.  Read fills the counts and rows
 * (tails cleared) and fails on a missing file, a file longer than its row or a .c.bin that is not 16 bytes.  Both block until done. */
PCCX_API size_t pccx_streams_packed_bytes(int B, int s_stride, int p_cap);
PCCX_API int pccx_write_streams_host(const void *packed_host, int B, int s_stride, int p_cap, const char *dir, const char *names,
                                     const int64_t *name_off, int threads);
PCCX_API int pccx_read_streams_host(void *packed_host, int B, int s_stride, int p_cap, const char *dir, const char *names,
                                    const int64_t *name_off, int threads);
/* Sizes in bytes of <name>.s.bin and <name>.p.bin of B clouds (-1 = no such file): what a reader sizes s_stride / p_cap from. */
PCCX_API int pccx_stream_sizes_host(int B, const char *dir, const char *names, const int64_t *name_off, int64_t *s_sizes,
                                    int64_t *p_sizes, int threads);

/* ---- generic layers for the other model families (PPPF_AE.py, pointnet_sa_module.py,
 *      pppe_pcd_ae.py:556-917): correctness-first building blocks ------------------------------- */

/* 1x1 Conv2d / Conv1d / Linear (pointnet_sa_module.py:51, PPPF_AE.py:65-80,122-123,
 * pppe_pcd_ae.py:556-568,697-707) on row-major "channels last" activations, with eval-mode
 * BatchNorm folded into W and b by the caller: out[M][N] = act(x[M][K] . W^T + b).
 * pccx_pack_linear (HOST pointers): W (N,K) row-major -> pccx_packed_linear_floats(N,K) floats.
 * pccx_linear: x (M, ldx>=K), wp packed (device), bias (N) or NULL, out (M, ldo>=N); `relu` is a flag word: bit 0 = ReLU,
 * bit 1 = the autocast form of train_pppe_pcd_ae.py:193-217 (operands and result rounded to bf16, products on the bf16
 * matrix cores, fp32 accumulate; pccx_linear_dw takes the same bit 1 in `flags`); bit 4 (16), with bit 1 only: operands rounded to
 * bf16 as above, the result stored in fp32 unrounded -- for a caller that adds the bias itself and then rounds once (the role-swapped
 * layers of pccx/train.py, whose bias runs along the output's rows). */
PCCX_API size_t pccx_packed_linear_floats(int N, int K);
PCCX_API int pccx_pack_linear(const float *W_host, int N, int K, float *wp_host);
PCCX_API int pccx_linear(const float *x, int M, int K, int ldx, const float *wp, const float *bias,
                         int N, int relu, float *out, int ldo, void *stream);

/* The same layer in the bf16x3 arithmetic: pccx_pack_linear_b3 splits the packed f32 fragments (device)
 * into three bf16 planes per K = 32 block, pccx_linear_b3 forms each fp32 product from six bf16 MFMA products, fp32 accumulate. */
PCCX_API size_t pccx_packed_linear_b3_floats(int N, int K);
PCCX_API int pccx_pack_linear_b3(const float *wp_dev, int N, int K, float *wplanes_dev, void *stream);
PCCX_API int pccx_linear_b3(const float *x, int M, int K, int ldx, const float *wplanes, const float *bias,
                            int N, int relu, float *out, int ldo, void *stream);

/* The wide stacks of the PointNet++ families kept in "planes" between layers (csrc/planes.hip): the activation of M rows x K
 * channels is stored as the three bf16 planes of the next layer's MFMA B operand, [K/32 block][16-row tile][plane][64 lanes] x 16 B,
 * pccx_planes_floats(M, K) floats.
 *   pccx_group_planes : gather + concat + split = index_points(features, idx) ++ index_points(xyz, idx) of
 *       pointnet_sa_module.py:73-83 (idx -1 -> row 0, :27), written as planes.  Row r reads source row
 *       (r / rows_per_batch) * n_src + idx[r] of f0 (C0 channels, row stride ld0) then f1 (C1, ld1); idx NULL: row r itself
 *       (fp32 rows -> planes).  Either source may be absent (C = 0).
 *   pccx_pack_planes_gemm : pccx_pack_linear_b3's planes reordered into per-m-block streams (pccx_planes_gemm_weight_floats).
 *   pccx_planes_gemm  : one Conv1x1 / Linear (+ folded BatchNorm) (+ ReLU, bit 0 of relu) on planes.  epilogue 0: out = planes of
 *       the N output channels; 1: out = fp32 rows (M, ldo); 2: out (M / group, ldo) = max over each `group` consecutive rows
 *       (torch.max over nsample, pointnet_sa_module.py:91; group in {16, 32, 64, 128} dividing M). */
PCCX_API size_t pccx_planes_floats(int64_t M, int K);
PCCX_API int pccx_group_planes(const float *f0, int C0, int ld0, const float *f1, int C1, int ld1, const int64_t *idx, int64_t M,
                               int64_t rows_per_batch, int64_t n_src, float *planes, void *stream);
/* The kNN grouping of the pppe set abstraction, pppe_pcd_ae.py:599-606 (index_points of xyz and features, the centre subtracted, xyz first),
 * written as the operand planes of the stack's first layer: row r = (b, s, j) holds offsets[r] = xyz[b, idx[r]] - centre[b, s] (M rows of 3
 * floats: pccx_knn_list's nn field with patch_scale 1) and feats[b * n_src + idx[r]] (C channels, row stride ldf; C = 0: no features, idx
 * unused).  The planes hold [C features | 3 offsets | zeros] -- the layout of pccx_group_planes -- so the first layer's weight columns are
 * permuted to match when it is packed; the (M, 3 + C) fp32 tensor of :606 never exists.  amax8 (device, 8 floats, or NULL): the largest
 * |offset| is folded into it as pccx_absmax does. */
PCCX_API int pccx_group_planes_centred(const float *feats, int C, int ldf, const float *offsets, const int64_t *idx, int64_t M,
                                       int64_t rows_per_batch, int64_t n_src, float *amax8, float *planes, void *stream);
/* torch.cat([a, b.unsqueeze(1).repeat(1, P, 1)], -1) written directly as planes (FoldingNet's inputs, PPPF_AE.py:99-106): row r =
 * the C0 channels of f0 row (mod0 > 0 ? r % mod0 : r) then the C1 channels of f1 row r / div1. */
PCCX_API int pccx_fold_planes(const float *f0, int C0, int ld0, int64_t mod0, const float *f1, int C1, int ld1, int64_t div1, int64_t M,
                              float *planes, void *stream);
/* act(base[r / div] + x[mod ? r % mod : r] @ w^T), r < M -- pccx_rows_affine_small's values (same fmaf chain) -- written as the operand
 * planes of the next layer (pccx_planes_floats(M, C) floats) instead of fp32 rows: FoldingNet's first layers, PPPF_AE.py:99-107 */
PCCX_API int pccx_rows_affine_planes(const float *base, int C, int64_t div, const float *x, int ldx, int Ks, int64_t mod, const float *w,
                                     int relu, int64_t M, float *planes, void *stream);
PCCX_API size_t pccx_planes_gemm_weight_floats(int N, int K);
PCCX_API int pccx_pack_planes_gemm(const float *wplanes_dev, int N, int K, float *wstream_dev, void *stream);
PCCX_API int pccx_planes_gemm(const float *planes_in, int64_t M, int K, const float *wstream, const float *bias, int N, int relu,
                              int epilogue, int group, float *out, int ldo, void *stream);
/* pccx_planes_gemm with the gather inside the kernel: row r of the input = row (r / rows_per_batch) * n_src + max(idx[r], 0) of src,
 * fp32 rows of ldp = 32 * ceil(K / 32) floats ([features, xyz] zero padded, 16-byte aligned). */
PCCX_API int pccx_planes_gemm_gather(const float *src, int ldp, const int64_t *idx, int64_t rows_per_batch, int64_t n_src, int64_t M,
                                     int K, const float *wstream, const float *bias, int N, int relu, int epilogue, int group,
                                     float *out, int ldo, void *stream);
/* Three wide Conv-BN-ReLU layers (widths 241..256, 241..256, 497..512: the first three of sa3, PPPF_AE.py:32-34) in one kernel, one
 * 16-row tile per wave, activations in registers, the input rows gathered inside (as pccx_planes_gemm_gather; idx NULL: row r itself);
 * the output is the operand planes of the layer that follows.  K0 of 8 or 9 blocks of 32 channels (<= 288).  The weight stream is
 * built by pccx_pack_planes_chain_wide from the three layers' pccx_pack_linear_b3 planes. */
PCCX_API size_t pccx_planes_chain_wide_weight_floats(int K0);
PCCX_API int pccx_pack_planes_chain_wide(const float *wp3_l0, const float *wp3_l1, const float *wp3_l2, int K0, int N0, int N1, int N2,
                                         float *wstream_dev, void *stream);
PCCX_API int pccx_planes_chain_wide(const float *src, int ldp, const int64_t *idx, int64_t rows_per_batch, int64_t n_src, int64_t M,
                                    int K0, const float *wstream, const float *b0, int N0, const float *b1, int N1, const float *b2,
                                    int N2, float *out_planes, void *stream);
/* A whole Conv-BN-ReLU x 4 + max-over-nsample stack (pointnet_sa_module.py:90-91) in one kernel, the activations between the layers
 * staying in registers: out (M / group, ldo) from the planes of the gathered input.  wstream = the four layers'
 * pccx_pack_planes_gemm streams back to back; b0..b3 the (folded) biases.  Supported width patterns: (<=32, 33..64, 33..64, 65..128)
 * and (97..128, 97..128, 97..128, 129..256) -- sa1 and sa2 of PPPF_AE.py:29-34; anything else returns PCCX_ERR_ARG and the caller
 * runs pccx_planes_gemm layer by layer.  group in {32, 64, 128}, or 1 = no reduction: out (M, ldo) holds the stack's output rows
 * (the stacks evaluated once per SOURCE row, the groups taking their maxima with pccx_gather_max). */
PCCX_API int pccx_planes_chain4(const float *planes_in, int64_t M, int K0, const float *wstream, const float *b0, int N0,
                                const float *b1, int N1, const float *b2, int N2, const float *b3, int N3, int group, float *out,
                                int ldo, void *stream);
/* The same stack with the gather inside the kernel: row r of the input is row (r / rows_per_batch) * n_src + max(idx[r], 0) of src,
 * fp32 rows of ldp = 32 * ceil(K0 / 32) floats (the K0 channels [features, xyz] zero padded; 16-byte aligned).  The grouped tensor of
 * pointnet_sa_module.py:73-83 is never materialised. */
PCCX_API int pccx_planes_chain4_gather(const float *src, int ldp, const int64_t *idx, int64_t rows_per_batch, int64_t n_src, int64_t M,
                                       int K0, const float *wstream, const float *b0, int N0, const float *b1, int N1,
                                       const float *b2, int N2, const float *b3, int N3, int group, float *out, int ldo, void *stream);

/* ---- the same layers in the f16x2 arithmetic (f16x2): every fp32 product formed from TWO fp16 pieces per operand, three
 * v_mfma_f32_16x16x32_f16 per fp32 product instead of bf16x3's six, planes of 4 bytes per value instead of 6.  fp16 has five exponent
 * bits, so every operand travels times an exact power of two: activations entering layer l times sigma_l (chosen by the host from
 * rigorous interval bounds of the stack, so that |sigma_l y| <= 2^15), weights times tau_l (max|W| tau <= 2^14); a layer's accumulator
 * is sigma_l tau_l (W y + b s).  The host passes each layer's bias as sigma_l tau_l b and the power-of-two ratios the kernels need:
 * rho = sigma for a kernel that splits fp32 rows, scale_out = sigma_next / (sigma tau) for a planes epilogue, 1 / (sigma tau) for a
 * row / max epilogue.  The bounds assume stack inputs of magnitude <= 1: `dyn` (device, 2 floats from pccx_dyn_scale: s and 1 / s, or
 * NULL for 1) is the stack's dynamic input normalisation -- Conv / ReLU stacks are positively homogeneous in (input, biases), so the
 * kernels multiply gathered inputs and biases by s and the stack's final rows by 1 / s; no input can overflow whatever the data.
 * amax8 (device, 8 floats, or NULL): the row epilogues fold the largest |value| they write into it (atomic max over 8 replicas) --
 * the next stack's input bound (for a max epilogue: pccx_planes_gemm_h2_max_amax).  Same shapes, epilogues and restrictions as the
 * bf16x3 entry points above. */
PCCX_API size_t pccx_planes_floats_h2(int64_t M, int K);
PCCX_API size_t pccx_packed_linear_h2_floats(int N, int K);
/* wp_dev: the f32 fragments of pccx_pack_linear (uploaded) -> the two fp16 planes [t][MT][2] of tau * W */
PCCX_API int pccx_pack_linear_h2(const float *wp_dev, int N, int K, float tau, float *wplanes_dev, void *stream);
PCCX_API size_t pccx_planes_gemm_weight_floats_h2(int N, int K);
PCCX_API int pccx_pack_planes_gemm_h2(const float *wplanes_dev, int N, int K, float *wstream_dev, void *stream);
PCCX_API int pccx_group_planes_h2(const float *f0, int C0, int ld0, const float *f1, int C1, int ld1, const int64_t *idx, int64_t M,
                                  int64_t rows_per_batch, int64_t n_src, float rho, const float *dyn, float *planes, void *stream);
PCCX_API int pccx_group_planes_centred_h2(const float *feats, int C, int ldf, const float *offsets, const int64_t *idx, int64_t M,
                                          int64_t rows_per_batch, int64_t n_src, float *amax8, float rho, const float *dyn, float *planes,
                                          void *stream);
PCCX_API int pccx_fold_planes_h2(const float *f0, int C0, int ld0, int64_t mod0, const float *f1, int C1, int ld1, int64_t div1, int64_t M,
                                 float rho, const float *dyn, float *planes, void *stream);
PCCX_API int pccx_rows_affine_planes_h2(const float *base, int C, int64_t div, const float *x, int ldx, int Ks, int64_t mod, const float *w,
                                        int relu, int64_t M, float rho, const float *dyn, float *planes, void *stream);
PCCX_API int pccx_planes_gemm_h2(const float *planes_in, int64_t M, int K, const float *wstream, const float *bias, int N, int relu,
                                 int epilogue, int group, float scale_out, const float *dyn, float *amax8, float *out, int ldo,
                                 void *stream);
/* The last layer of a set-abstraction stack whose groups are only reduced together (PPPF_AE.py:44 over pointnet_sa_module.py:91: the maximum
 * over the centroids of the maxima over their samples = the maximum over every source row that is a sample of any centroid, because the stack
 * acts on each un-centred row by itself): member = 1 byte per row from pccx_group_members, group = the source rows of one batch element
 * (32, 64 or 128, M % group == 0) -> out (M / group, ldo).  The layer's fp32 rows are never written. */
PCCX_API int pccx_planes_gemm_h2_member_max(const float *planes_in, int64_t M, int K, const float *wstream, const float *bias, int N, int relu,
                                            int group, const unsigned char *member, float scale_out, const float *dyn, float *out, int ldo,
                                            void *stream);
/* The last layer of a pppe set-abstraction stack (the max over the K neighbours, pppe_pcd_ae.py:607-610): pccx_planes_gemm_h2's max epilogue
 * (group in {16, 32, 64, 128}, M % group == 0 -> out (M / group, ldo)) that also folds the largest |maximum| it writes into amax8 (required):
 * the bound of the next level's input features. */
PCCX_API int pccx_planes_gemm_h2_max_amax(const float *planes_in, int64_t M, int K, const float *wstream, const float *bias, int N, int relu,
                                          int group, float scale_out, const float *dyn, float *amax8, float *out, int ldo, void *stream);
/* member (n_idx / per_batch, n_src) bytes: 1 where the row is named by an entry of idx (per_batch entries per batch element; -1 -> row 0, the
 * clamp of pointnet_sa_module.py:27), else 0.  The table's size and address must be multiples of 4 (cleared in words by a kernel). */
PCCX_API int pccx_group_members(const int64_t *idx, int64_t n_idx, int64_t per_batch, int64_t n_src, unsigned char *member, void *stream);
PCCX_API int pccx_planes_gemm_gather_h2(const float *src, int ldp, const int64_t *idx, int64_t rows_per_batch, int64_t n_src, int64_t M,
                                        int K, const float *wstream, const float *bias, int N, int relu, int epilogue, int group,
                                        float rho_in, float scale_out, const float *dyn, float *amax8, float *out, int ldo,
                                        void *stream);
/* scales5_host (HOST, 5 floats): {rho_in (gather form only), rho_1, rho_2, rho_3, 1 / (sigma_3 tau_3)}, rho_l = sigma_l / (sigma_{l-1} tau_{l-1}) */
PCCX_API int pccx_planes_chain4_h2(const float *planes_in, int64_t M, int K0, const float *wstream, const float *b0, int N0,
                                   const float *b1, int N1, const float *b2, int N2, const float *b3, int N3, int group,
                                   const float *scales5_host, const float *dyn, float *amax8, float *out, int ldo, void *stream);
PCCX_API int pccx_planes_chain4_gather_h2(const float *src, int ldp, const int64_t *idx, int64_t rows_per_batch, int64_t n_src, int64_t M,
                                          int K0, const float *wstream, const float *b0, int N0, const float *b1, int N1,
                                          const float *b2, int N2, const float *b3, int N3, int group, const float *scales5_host,
                                          const float *dyn, float *amax8, float *out, int ldo, void *stream);
/* The dynamic input normalisation: pccx_absmax folds max |x| over n floats into amax8 (8 non-negative floats the caller cleared);
 * pccx_dyn_scale turns one or two such maxima into dyn2 = {s, 1 / s}, s the largest power of two <= 1 with bound * s <= 1 where
 * bound = (combine ? max(a1 m1, a2 m2) : a1 m1 + a2 m2) + add (m2_8 may be NULL). */
PCCX_API int pccx_absmax(const float *x, int64_t n, float *amax8, void *stream);
PCCX_API int pccx_dyn_scale(const float *m1_8, float a1, const float *m2_8, float a2, float add, int combine, float *dyn2, void *stream);

/* The epilogue of pccx_prob_forward as an op of its own, for the generic (any --d / --L, compress.py:30-34) path: softmax over
 * the L levels of each row of logits (rows, L), pmf_to_cdf (pn_kit.py:452-461: cumsum, leading 0, clamp <= 1) and torchac 0.9.3's
 * integer CDF.  Any of pmf (rows, L), cdf (rows, L+1), cdf_int (rows, L+1) may be NULL. */
PCCX_API int pccx_softmax_cdf(const float *logits, int64_t rows, int L, float *pmf, float *cdf, int32_t *cdf_int, void *stream);
/* The reassembly epilogue of pccx_ae_decode as an op of its own (decompress.py:104-116): patches (P, k, 3) raw decoder output ->
 * out (P*k, 3) = ((patch / scale) + centres[patch] - 0.5) * longest[b] / (1 - margin) + center[b], b = patch / S. */
PCCX_API int pccx_reassemble(const float *patches, int64_t P, int k, float scale, const float *centres, const float *nrm_center,
                             const float *nrm_longest, int S, double margin, float *out, void *stream);

/* ---- ragged batches: clouds of different sizes in one launch sequence (octree mode "full") ----------------
 * Cloud b holds n[b] points in the first rows of its (N_max, 3) slab and S[b] = n[b]*ALPHA/K centres in the first rows of its
 * (S_max, 3) slab; the rows behind them are padding whose contents never reach a result.  The per-cloud counts and scales are
 * device arrays of B entries.  Each entry is its dense namesake with the count taken per cloud: the same operations in the same
 * order, so what cloud b gets is bit for bit what the dense entry gives on the unpadded cloud alone.  A count outside its range is
 * clamped into it by the kernels (they never index out of a slab); the host layer refuses such a batch before any launch.
 *
 * pccx_normalize_n: the box over the rows < n[b]; out rows from n[b] on are written as zeros.
 * pccx_fps_n: cloud b runs npoint[b] <= npoint_max rounds over its n[b] points; idx_out (B, npoint_max), the entries from
 *   npoint[b] on repeat the last selected index.  N_max <= 32768; workspace: B*N_max floats when N_max > 16384, else may be NULL.
 * pccx_octree_encode_n: pccx_octree_encode with each cloud's own S[b] and N[b] in the depth search; rows >= S[b] are not read;
 *   the strides of bits / bytes are those of pccx_octree_bits_capacity(S_max).  S_max <= 1024.
 * pccx_knn_list_n: pccx_knn_list with N -> n[b] (K <= n[b]) and patch_scale -> scale[b]; the kernel is chosen by N_max.
 * pccx_range_encode_n / pccx_range_decode_n: nsym is the row stride of cdf_int / latent_q in symbols; cloud b codes or decodes its
 *   first nsym_of[b] <= nsym symbols from a fresh state and flushes as pccx_range_encode does: the bytes are that entry's on the
 *   same table and symbols.  Decode writes zeros behind them; foreign bytes are taken as pccx_range_decode takes them.  The kernel
 *   form is pccx_range_coder_form's for the row.
 * pccx_reassemble_n: pccx_reassemble's formula with scale[b] on the patches < S[b] of cloud b; patches (B*S_max, k, 3) -> out
 *   (B, S_max*k, 3), of which the rows from S[b]*k on are not written. */
PCCX_API int pccx_normalize_n(const float *pc, int B, int N_max, const int32_t *n, double margin, float *out, float *center,
                              float *longest, void *stream);
PCCX_API int pccx_fps_n(const float *xyz, int B, int N_max, const int32_t *n, int npoint_max, const int32_t *npoint,
                        const int32_t *start_idx, int64_t *idx_out, float *workspace, void *stream);
PCCX_API int pccx_octree_encode_n(const float *centres, int B, int S_max, const int32_t *S, const int32_t *N, double min_bpp,
                                  uint8_t *bits, int32_t *nbits, int32_t *depth, uint8_t *bytes, int32_t *nbytes, void *stream);
PCCX_API int pccx_knn_list_n(const float *q, int B, int M, const float *ref, int N_max, const int32_t *n, int K, float *dists,
                             int64_t *idx, float *nn, const float *scale, const int32_t *rep, void *stream);
PCCX_API int pccx_range_encode_n(const int32_t *cdf_int, const float *latent_q, int B, int nsym, const int32_t *nsym_of, int L,
                                 uint8_t *out, int cap, int32_t *nbytes, void *stream);
PCCX_API int pccx_range_decode_n(const int32_t *cdf_int, const uint8_t *in, int stride, const int32_t *nbytes, int B, int nsym,
                                 const int32_t *nsym_of, int L, float *latent_q, void *stream);
PCCX_API int pccx_reassemble_n(const float *patches, int B, int S_max, const int32_t *S, int k, const float *scale,
                               const float *centres, const float *nrm_center, const float *nrm_longest, double margin, float *out,
                               void *stream);

/* out[r][c] = act(base[r / div][c] + sum_{k<Ks} x[(mod ? r % mod : r)][k] * w[c][k]), Ks <= 4, C % 4 == 0: the per-point part of a
 * layer whose input rows are [small per-point part | long per-patch part] (FoldingNet's [grid | latent] and [coarse | latent],
 * PPPF_AE.py:99-107); base = the per-patch part's Linear (bias included), one row per patch.  w is (C, Ks) row-major. */
PCCX_API int pccx_rows_affine_small(const float *base, int C, int64_t div, const float *x, int ldx, int Ks, int64_t mod,
                                    const float *w, int relu, int64_t M, float *out, void *stream);
/* torch.max(knn_gather(y, idx.clamp(min=0)), nsample_dim)[0] without the gathered tensor (pointnet_sa_module.py:27-28,91):
 * y (B,N,C) fp32 rows, idx (B,M,ns) int64 with -1 padding -> out (B,M,C).  C % 4 == 0.  With it PointnetSAModule (which gathers
 * un-centred rows, :73-85) runs its Conv-BN-ReLU stack on the N source rows once instead of on M*ns copies of them. */
PCCX_API int pccx_gather_max(const float *y, int B, int N, int C, const int64_t *idx, int M, int ns, float *out, void *stream);
/* The same maxima written as the NEXT level's input rows (pointnet_sa_module.py:83, features first, xyz last): out (B, M, ldo),
 * ldo = 32 * ceil((C + 3) / 32): [C maxima | xyz (B, M, 3) of the centroids | zeros] -- what the gathering planes kernels read. */
PCCX_API int pccx_gather_max_rows(const float *y, int B, int N, int C, const int64_t *idx, int M, int ns, const float *xyz, float *out, int ldo,
                                  void *stream);
/* torch.max(features, neighbour_dim)[0] (pointnet_sa_module.py:91, pppe_pcd_ae.py:610):
 * x (G,Kn,C) -> out (G,C). */
PCCX_API int pccx_group_max(const float *x, int64_t G, int Kn, int C, float *out, void *stream);

/* y = sigmoid(x)*(L-0.2) - (L-0.2)/2 (PPPF_AE.py:136-137, AE.py:43-44), optionally rounded;
 * y = round(x) (AE.STEQuantize, AE.py:79-81). */
PCCX_API int pccx_sigmoid_spread(const float *x, int64_t n, int L, int do_round, float *y, void *stream);
PCCX_API int pccx_round(const float *x, int64_t n, float *y, void *stream);

/* quantize_st forward value and its dequantisation (pppe_pcd_ae.py:719-735, :873). y_deq may be NULL. */
PCCX_API int pccx_quantize_st(const float *x, int64_t n, float qmin, float qmax, int levels, float *y_q,
                              float *y_deq, void *stream);

/* ---- training-step primitives (train_pppe_pcd_ae.py:184-226): train-mode BatchNorm, the
 *      backward of the generic layers, loss pieces, gradient clipping and Adam.  Rows are channels-last.
 *      `sums` arguments are scratch of 2*C doubles. ------------------------------------------------ */
PCCX_API int pccx_pack_linear_device(const float *W, int N, int K, int transpose, float *wp, void *stream);
/* dW (N,K) += dZ^T (M,N) . X (M,K)   (dW must be initialised by the caller) */
PCCX_API int pccx_linear_dw(const float *dZ, const float *X, int64_t M, int N, int K, int ldz, int ldx,
                            float *dW, int flags, void *stream);
/* BatchNorm{1,2}d in training mode (pppe_pcd_ae.py:556-568): batch moments per channel, running stats
 * updated with `momentum` (running_* may be NULL); then y = [relu]((z-mean)*rstd*gamma+beta). */
PCCX_API int pccx_bn_train_stats(const float *Z, int64_t M, int C, float eps, float momentum, double *sums,
                                 float *mean, float *rstd, float *running_mean, float *running_var,
                                 void *stream);
PCCX_API int pccx_bn_relu_forward(const float *Z, int64_t M, int C, const float *mean, const float *rstd,
                                  const float *gamma, const float *beta, int relu, float *Y, void *stream);
/* backward of BN(train)+ReLU: dZ, and g_gamma / g_beta ACCUMULATED into the parameter gradients */
PCCX_API int pccx_bn_relu_backward(const float *dY, const float *Y, const float *Z, int64_t M, int C,
                                   const float *mean, const float *rstd, const float *gamma, double *sums,
                                   float *dZ, float *g_gamma, float *g_beta, void *stream);
/* nn.Linear on 1..8 rows (the pppe model's global, decoder and probability Linears at batch 4, pppe_pcd_ae.py:655-714, :739-802):
 * out (M, N) = act(x (M, K) . W^T + b) and dX (M, K) += dZ (M, N) . W straight from the row-major W (N, K), each W row read once
 * (a weight stream, not matrix work; no packed copy).  flags as pccx_linear (bit 0 ReLU, bit 1 autocast rounding).  K % 4 == 0;
 * dX is zeroed by the caller. */
PCCX_API int pccx_linear_skinny(const float *x, int M, int K, int ldx, const float *W, const float *bias, int N, int flags,
                                float *out, int ldo, void *stream);
PCCX_API int pccx_linear_skinny_dx(const float *dZ, int M, int N, int ldz, const float *W, int K, int flags, float *dX, int ldd,
                                   void *stream);
PCCX_API int pccx_col_sum(const float *dY, int64_t M, int C, double *sums, float *g_bias, void *stream);
/* The training step's forms of the four entry points above (train_pppe_pcd_ae.py:184-226; round 4): the same arithmetic in fewer launches.
 * flags bit 2 (value 4): the accumulation target (`sums`, dF, gX / gY) was CLEARED BY THE CALLER -- pccx/train.py clears one arena per
 * step with pccx_zero_bytes instead of one launch per reduction; pccx_bn_relu_train_forward flags bit 3 (value 8): `sums` already HOLDS the
 * column moments of Z (pccx_linear_moments produced Z), no reduction is launched; likewise pccx_bn_relu_train_backward after pccx_linear_bnback.  pccx_bn_relu_train_forward = pccx_bn_train_stats + pccx_bn_relu_forward
 * (moments, then one kernel that finalises them and applies the layer; mean / rstd / running stats / Y bit-identical);
 * pccx_bn_relu_train_backward = pccx_bn_relu_backward with g_gamma / g_beta WRITTEN (not accumulated); pccx_col_sum_w writes g_bias. */
PCCX_API int pccx_bn_relu_train_forward(const float *Z, int64_t M, int C, float eps, float momentum, double *sums, const float *gamma,
                                        const float *beta, int relu, float *mean, float *rstd, float *running_mean,
                                        float *running_var, float *Y, int flags, void *stream);
PCCX_API int pccx_bn_relu_train_backward(const float *dY, const float *Y, const float *Z, int64_t M, int C, const float *mean,
                                         const float *rstd, const float *gamma, double *sums, float *dZ, float *g_gamma,
                                         float *g_beta, int flags, void *stream);
PCCX_API int pccx_col_sum_w(const float *dY, int64_t M, int C, double *sums, float *g_bias, int flags, void *stream);
/* `sums` of the three entry points above holds pccx_train_sums_doubles(C) doubles (eight replicas of the 2 C column sums: a workgroup adds
 * into replica blockIdx % 8, the consuming kernel adds the replicas up -- the same-address atomics at the end of a reduction are an eighth
 * as deep); the older pccx_bn_train_stats / pccx_bn_relu_backward / pccx_col_sum keep their 2 C doubles. */
PCCX_API size_t pccx_train_sums_doubles(int C);
/* A Conv / Linear without bias whose epilogue accumulates the column moments of its output (sum z, sum z^2 into the eight replicas of
 * `sums`, pccx_train_sums_doubles(N) doubles): the Conv -> BatchNorm pairs of pppe_pcd_ae.py:556-568 in train mode then need no pass of
 * their own over the activation -- pccx_bn_relu_train_forward with flags bit 3 (8) takes `sums` as filled.  flags: bit 1 (2) = autocast
 * (bf16 operands and result; the moments are those of the rounded result), bit 2 (4) = `sums` was cleared by the caller. */
PCCX_API int pccx_linear_moments(const float *x, int M, int K, int ldx, const float *wp, int N, int flags, float *out, int ldo,
                                 double *sums, void *stream);
/* The dX GEMM behind such a pair in the backward pass: out = x . W^T is the BatchNorm's dY, and the epilogue accumulates the two column
 * sums its backward needs (sum d xhat | sum d, d = (Y > 0 ? dY : 0), xhat = (Z - mean) rstd) from the rows it has just produced;
 * pccx_bn_relu_train_backward with flags bit 3 (8) takes `sums` as filled.  Y, Z: the BatchNorm's output and input rows (M, ldo). */
PCCX_API int pccx_linear_bnback(const float *x, int M, int K, int ldx, const float *wp, int N, int flags, float *out, int ldo,
                                const float *Y, const float *Z, const float *mean, const float *rstd, double *sums, void *stream);
/* clear `bytes` (a multiple of 4) with a kernel (as a hipGraph node it is ordered like every other kernel: DESIGN.md section 7) */
PCCX_API int pccx_zero_bytes(void *p, size_t bytes, void *stream);
/* dst[0 .. bytes) = src[0 .. bytes) by a kernel (both 16-byte aligned, bytes % 16 == 0): how a training loop hands the next batch and its
 * FPS / kNN tables (functions of the coordinates only, pppe_pcd_ae.py:596-632) to the fixed buffers a captured step reads. */
PCCX_API int pccx_copy_bytes(const void *src, void *dst, size_t bytes, void *stream);
/* *table[i] += delta for n int64 counters whose device addresses sit in table_dev (BatchNorm's num_batches_tracked of a whole model) */
PCCX_API int pccx_add_i64_table(const int64_t *table_dev, int n, int64_t delta, void *stream);
PCCX_API int pccx_relu_backward(const float *dY, const float *Y, int64_t n, float *dZ, void *stream);
PCCX_API int pccx_group_max_arg(const float *x, int64_t G, int Kn, int C, float *out, int32_t *arg,
                                void *stream);
PCCX_API int pccx_group_max_backward(const float *dOut, const int32_t *arg, int64_t G, int Kn, int C,
                                     float *dX, void *stream);
/* backward of pccx_gather: dF (B,N,C) = scatter-add of dG (B,Mrows, row stride ldg >= C) through idx */
PCCX_API int pccx_gather_backward(const float *dG, int ldg, const int64_t *idx, int B, int Mrows, int N,
                                  int C, float *dF, void *stream);
/* the same, ACCUMULATING into a dF the caller cleared (flags & 4; without the flag dF is cleared here) */
PCCX_API int pccx_gather_backward_acc(const float *dG, int ldg, const int64_t *idx, int B, int Mrows, int N, int C, float *dF,
                                      int flags, void *stream);
/* F.smooth_l1_loss(a, b, reduction="mean") * n summed into value[0] (double); grad = grad_scale * dl/da */
PCCX_API int pccx_smooth_l1(const float *a, const float *b, int64_t n, float grad_scale, double *value,
                            float *grad, void *stream);
PCCX_API int pccx_quantize_st_backward(const float *x, const float *d_ydeq, int64_t n, float qmin, float qmax,
                                       int levels, float *dx, void *stream);
PCCX_API int pccx_rate_from_logits(const float *logits, const float *y_q, int B, int bins, int ld_yq,
                                   float *out, void *stream);
/* clip_grad_norm_ + torch.optim.Adam: accumulate sum g^2 over all tensors into acc (zeroed by the caller),
 * then one pccx_adam_step per tensor reads the norm on the device (gnorm_sq may be NULL = no clipping).  The betas are doubles:
 * 1 - beta and 1 - beta^step are formed in double and rounded to float once, as torch.optim.Adam forms them. */
PCCX_API int pccx_sumsq_accumulate(const float *g, int64_t n, double *acc, void *stream);
PCCX_API int pccx_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                            const double *gnorm_sq, float max_norm, float lr, double beta1, double beta2,
                            float eps, int step, void *stream);
/* The same two steps over ALL parameter tensors in one launch each.  table_dev: ntensors rows of six int64 in device memory,
 * {param, grad, exp_avg, exp_avg_sq (device pointers), n (elements), first_block}; a workgroup handles 1024 consecutive elements
 * of one tensor, first_block = sum over the earlier rows of ceil(n / 1024), total_blocks = that sum over all rows.  hyper_dev
 * (the device state below) replaces lr / step when not NULL.  Element for element the arithmetic of pccx_adam_step. */
PCCX_API int pccx_sumsq_multi(const int64_t *table_dev, int ntensors, int64_t total_blocks, double *acc, void *stream);
PCCX_API int pccx_adam_multi(const int64_t *table_dev, int ntensors, int64_t total_blocks, const double *gnorm_sq,
                             float max_norm, const float *hyper_dev, float lr, int step, double beta1, double beta2,
                             float eps, void *stream);
/* Adam's per-step scalars kept on the device (torch.optim.Adam's `step` / bias_correction1/2, train_pppe_pcd_ae.py:216,220 via
 * optimizer.step()): a 32-byte, 8-byte aligned state
 *     float lr | float 1-beta1^t | float 1-beta2^t | int32 t | double beta1^t | double beta2^t
 * pccx_adam_advance_dev does t += 1 and refreshes the two corrections (one thread, stream-ordered), so a captured training
 * step carries its own step counter and a replay needs no host write. */
PCCX_API int pccx_adam_advance_dev(float *hyper, double beta1, double beta2, void *stream);
/* pccx_adam_step with lr and the bias corrections read from that device state (its first three floats).
 * No per-step launch argument, so the training step can be captured as a hipGraph (pccx.train.GraphedTrainStep). */
PCCX_API int pccx_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                const double *gnorm_sq, float max_norm, const float *hyper, double beta1, double beta2,
                                float eps, void *stream);

/* ---- 11b. The deterministic mode of the training step (pccx.train.step_scope(deterministic=True)): every accumulation of a
 *      step in a FIXED order, so that a step is a pure function of its inputs and bit-identical from run to run.  Each entry WRITES its
 *      result (no cleared buffer is needed, what the output held is ignored) and takes its scratch from the caller; every launch geometry
 *      is a function of the shapes alone.  Workspaces are plain uninitialised memory of the size the *_workspace_* / *_doubles call names. */
/* (a) stands in for pccx_linear_dw (also with the roles swapped, pccx/train.py _is_wide): every row slice stores its partial dW tile in
 * workspace [slices][N][K], a second kernel adds the slices in ascending index.  The workspace is at most max(8 N K, 2 Mi) floats; a
 * shape that splits into one slice needs none (the size is then 0 and workspace may be NULL). */
PCCX_API size_t pccx_linear_dw_det_workspace_floats(int64_t M, int N, int K);
PCCX_API int pccx_linear_dw_det(const float *dZ, const float *X, int64_t M, int N, int K, int ldz, int ldx, float *dW, int flags,
                                float *workspace, void *stream);
/* (a) stands in for pccx_linear_skinny_dx: the n-chunks store their partial rows in workspace [chunks][M][K] (16-byte aligned, at most
 * a quarter of the weight), added in ascending chunk index. */
PCCX_API size_t pccx_linear_skinny_dx_det_workspace_floats(int M, int N, int K);
PCCX_API int pccx_linear_skinny_dx_det(const float *dZ, int M, int N, int ldz, const float *W, int K, int flags, float *dX, int ldd,
                                       float *workspace, void *stream);
/* (b) stands in for the column reductions inside pccx_bn_relu_train_forward (mode 0: sum z, sum z^2 of A), pccx_bn_relu_train_backward
 * (mode 1: sum dy (y>0) xhat, sum dy (y>0) with dY = A) and pccx_col_sum_w (mode 2: sum of A), and for the epilogues of
 * pccx_linear_moments / pccx_linear_bnback, for any C: workgroup w stores its double partials in slot w of `partials`
 * (pccx_col_reduce_det_doubles(M, C) doubles), one kernel adds the slots in ascending index from +0.  sums (modes 0, 1;
 * pccx_train_sums_doubles(C) doubles, all written: totals in replica 0, +0 in the others) is what the two BatchNorm entries take with
 * flags 4 | 8; in mode 2 `sums` is C doubles.  f32_out: the first sum as C floats (the bias gradient).  Either may be NULL, not both. */
PCCX_API size_t pccx_col_reduce_det_doubles(int64_t M, int C);
PCCX_API int pccx_col_reduce_det(int mode, const float *A, const float *Y, const float *Z, const float *mean, const float *rstd,
                                 int64_t M, int C, double *partials, double *sums, float *f32_out, void *stream);
/* (b) stand in for pccx_smooth_l1 and pccx_sumsq_multi: value[0] / acc[0] WRITTEN as the sum of the workgroups' partials in ascending
 * workgroup index.  (pccx_rate_from_logits is one thread's loop: it has no order to fix.) */
PCCX_API size_t pccx_smooth_l1_det_doubles(int64_t n);
PCCX_API int pccx_smooth_l1_det(const float *a, const float *b, int64_t n, float grad_scale, double *partials, double *value,
                                float *grad, void *stream);
PCCX_API size_t pccx_sumsq_multi_det_doubles(int64_t total_blocks);
PCCX_API int pccx_sumsq_multi_det(const int64_t *table_dev, int ntensors, int64_t total_blocks, double *partials, double *acc,
                                  void *stream);
/* (c) stands in for pccx_gather_backward_acc: out (B,N,C) WRITTEN, out[b][n] = the fp32 sum from +0 of vals[b][m] (row stride ldv >= C)
 * over the m with idx[b][m] == n in ascending m; untouched rows are +0 (np.add.at on float32, bit for bit).  idx (B,Mrows): int64
 * (idx_is_i32 = 0) or int32 (1), clamped to [0, N-1].  The inverse lists are built on the device, no host read-back; a segment may be
 * as long as Mrows.  workspace: pccx_scatter_add_ordered_workspace_ints(B, Mrows, N) int32. */
PCCX_API size_t pccx_scatter_add_ordered_workspace_ints(int B, int Mrows, int N);
PCCX_API int pccx_scatter_add_ordered(const float *vals, int ldv, const void *idx, int idx_is_i32, int B, int Mrows, int N, int C,
                                      float *out, int32_t *workspace, void *stream);
/* (c) stands in for pccx_chamfer_grad_dev_acc: gX / gY WRITTEN; the nearest-neighbour scatter goes through pccx_scatter_add_ordered
 * (gX[i] = own term - ordered sum over the y that chose x_i). */
PCCX_API size_t pccx_chamfer_grad_det_workspace_floats(int B, int P, int Q);
PCCX_API size_t pccx_chamfer_grad_det_workspace_ints(int B, int P, int Q);
PCCX_API int pccx_chamfer_grad_det(const float *X, int B, int P, const float *Y, int Q, const int32_t *nn_xy, const int32_t *nn_yx,
                                   const float *grad_out_dev, float *gX, float *gY, float *ws_floats, int32_t *ws_ints, void *stream);

/* ---- training crops (csrc/crop.hip) --------------------------------------------------------------------------------------
 * Stands in for the reference's loader (train.py:110-123: every file holds exactly N points and is one sample); the reference itself
 * has no crop.  The store: every training cloud concatenated, points (M_total,3) f32, with offsets (F+1) int64 (cloud c = rows
 * offsets[c]..offsets[c+1]).  Slot b cuts from cloud cloud[b] the n[b] points with the smallest keys
 * (__float_as_uint(squared distance to point seed[b] of that cloud), index) -- ties in distance go to the lower index -- and writes
 * them in ascending index: out (B,N_cap,3) f32 with the rows behind n[b] NaN (codec.pad_clouds' convention), out_idx (B,N_cap) int32
 * with -1 behind n[b] (may be NULL).  cloud / seed / n: (B) int32 on the device, never read back, clamped where they are read (cloud
 * into [0,F-1], seed into [0,M-1], n into [1,min(N_cap,M)]); M_max: the largest cloud's point count, it sizes the grids together with B.
 * Limits, checked before any launch: M_max <= 16777216, N_cap <= 131072, B <= 1024.  Integer atomics only: the result does not depend
 * on scheduling.  No memset / memcpy: capturable, and every grid depends on (B, M_max) alone, so a captured call replays on other
 * tables.  workspace: pccx_crop_nearest_workspace_bytes(B, M_max) bytes, 8-byte aligned; its content on entry does not matter. */
PCCX_API size_t pccx_crop_nearest_workspace_bytes(int B, int M_max);
PCCX_API int pccx_crop_nearest(const float *points, int64_t M_total, const int64_t *offsets, int F, const int32_t *cloud,
                               const int32_t *seed, const int32_t *n, int B, int N_cap, int M_max, float *out, int32_t *out_idx,
                               void *workspace, void *stream);

/* ---- ragged evaluation (csrc/eval_metrics.hip) ---------------------------------------------------------------------------
 * eval.py's metrics over a padded slab of clouds of different sizes.  Every count table is (B) int32 ON THE DEVICE, never read back,
 * and clamped into [0, capacity] where a kernel reads it; rows behind a count are never loaded (they may hold NaN), outputs behind a
 * count stay unwritten, and a zero count forms no address into the slab.  B = 0 returns PCCX_OK with nothing launched; a null
 * pointer or a bad shape returns PCCX_ERR_ARG before any launch.  B <= 65535.
 * pccx_minmax_n: out (B,2,3) f32 = per-axis min (row 0) and max (row 1) of the first p[b] rows of X (B,P_max,3): amin / amax of the
 *   unpadded cloud, bit for bit.  A zero count gives (+inf, -inf).
 * pccx_query_rep_n: rep (B*M) int32 with rep[b*M+i] = b*M+i for i < n[b], else b*M -- handed to pccx_knn_list_n it keeps the padded
 *   queries of a slab from being searched (their output rows stay unwritten).  B*M < 2^31.
 * pccx_estimate_normals_n: pccx_estimate_normals on the rows < n[b] of xyz (B,N_max,3) with nbr (B,N_max,K) int64, whose rows behind
 *   n[b] are never read: cloud b's normals are the dense entry's on the unpadded cloud, bit for bit.
 * pccx_point_errors_n: D1 and D2 from one all-pairs scan.  d2 (B,P_max): pccx_nn_dist_n's values.  normals_Y (B,Q_max,3) and plane
 *   (B,P_max) come together or are both NULL: plane[b,i] = pccx_point_plane_err's value for the nearest row of Y (first minimum, lowest
 *   index among equal distances), taken from the scan's registers -- no argmin table is written.
 * pccx_mean_var_n: out (B,2) f64 = mean and population variance of the first p[b] entries of v (B,P_max) f32; two passes in double,
 *   one workgroup per cloud, a summation order fixed by p[b] alone (no atomics): a cloud's two numbers do not depend on the batch, its
 *   position in it or P_max.  A zero count gives NaN. */
PCCX_API int pccx_minmax_n(const float *X, int B, int P_max, const int32_t *p, float *out, void *stream);
PCCX_API int pccx_query_rep_n(const int32_t *n, int B, int M, int32_t *rep, void *stream);
PCCX_API int pccx_estimate_normals_n(const float *xyz, int B, int N_max, const int32_t *n, const int64_t *nbr, int K, float *normals,
                                     void *stream);
PCCX_API int pccx_point_errors_n(const float *X, int B, int P_max, const int32_t *p, const float *Y, const float *normals_Y, int Q_max,
                                 const int32_t *q, float *d2, float *plane, void *stream);
PCCX_API int pccx_mean_var_n(const float *v, int B, int P_max, const int32_t *p, double *out, void *stream);

/* ---- PLY files in and out (csrc/ply_host.h, csrc/hostio.hip, csrc/plyio.hip) ----------------------------------
 * Stands in for pn_kit.read_point_cloud / save_point_cloud (pn_kit.py:25-42) over a batch of files: headers and raw vertex blocks on
 * host threads, conversion to float32 on the GPU, the same arrays and the same files bit for bit.
 * Paths and names are packed as the stream functions take names: zero-terminated strings in one block, path_off[b] = where b's begins.
 * table (B, PCCX_PLY_ROW) int64 on the HOST, one row per file: 0 status (0 = good, else csrc/ply_host.h PlyStatus), 1 format (0 ascii,
 *   1 binary_little_endian, 2 binary_big_endian), 2 n_vertex, 3 record stride in bytes, 4 byte offset of the vertex data, 5 file size,
 *   6..8 byte offset of x y z inside a record, 9..11 their type codes (0 int8, 1 uint8, 2 int16, 3 uint16, 4 int32, 5 uint32, 6 float32,
 *   7 float64), 12 scalar properties per vertex, 13..15 property index of x y z.  msgs (B, msg_stride) chars: the cause, for every row
 *   whose status is not 0.  A file that fails does not stop the others, and both calls return PCCX_OK then: the caller reads the statuses.
 * pccx_ply_scan_host: opens every file, parses its header (limits: 1 <= n_vertex <= 2^31 - 1, stride <= 4096, the vertex block must
 *   fit the file, no element in front of vertex, no list property on it, no property name twice in a binary file) and fills its row.
 *   A header longer than the 4 KiB read first is read again, four times as far, up to 16 MiB.
 * pccx_ply_load_host: for every row with status 0, the vertex block -- n_vertex * stride bytes, nothing else, unconverted -- to
 *   staging_host + dst_off[b] (dst_off[b] a multiple of 16; staging_host 16-byte aligned).  An ASCII file is parsed by its thread (every
 *   token to double, then rounded to float, as np.loadtxt + astype do; no locale; inf and nan accepted) into n_vertex records of 12 bytes,
 *   float32 x y z, and its row is rewritten to say so (format 1, stride 12, offsets 0 4 8, type 6); fewer than n_vertex complete rows
 *   are refused.  Nothing outside [dst_off[b], dst_off[b] + n_vertex * (12 or stride)) is written.
 * pccx_ply_write_host: <dir>/<name><suffix> for B clouds, cloud b = rows first_row[b] .. + count[b] of rows_host (rows, 3) f32 on the
 *   HOST: plyio.save_point_cloud's bytes (its four header lines, little-endian float32), an existing file opened first as the stream
 *   files are.
 * threads: 0 = min(8, hardware threads), as above.
 * pccx_ply_unpack (GPU): staging = the device copy of the staging buffer (16-byte aligned, staging_bytes a multiple of 16); table
 *   (B, 12) int64 ON THE DEVICE: source byte offset, stride, byte offset of x y z, type code of x y z, big endian (0 / 1), n, dst_row,
 *   cap; tile_prefix (B + 1) int32 on the device = exclusive prefix of ceil(cap[b] / 256), total_tiles = its last entry.  Writes rows
 *   dst_row[b] .. + n[b] of out (rows, 3) f32 with cloud b's x y z converted as numpy's astype(float32) does (float32 copied bit for bit,
 *   float64 / int32 / uint32 rounded to nearest even) and rows n[b] .. cap[b] with the quiet NaN 0x7FC00000 of codec.pad_clouds.  dst_row
 *   = b * N_cap, cap = N_cap gives the padded slab; dst_row = offsets[b], cap = n[b] the packed store of codec.pack_clouds.  Every table
 *   field is clamped where it is read, against staging_bytes and rows too.  One kernel, no memset / memcpy: capturable. */
#define PCCX_PLY_ROW 16
PCCX_API int pccx_ply_scan_host(int B, const char *paths, const int64_t *path_off, int64_t *table, char *msgs, int msg_stride, int threads);
PCCX_API int pccx_ply_load_host(int B, const char *paths, const int64_t *path_off, int64_t *table, void *staging_host,
                                int64_t staging_bytes, const int64_t *dst_off, char *msgs, int msg_stride, int threads);
PCCX_API int pccx_ply_write_host(const float *rows_host, int64_t rows, const int64_t *first_row, const int64_t *count, int B,
                                 const char *dir, const char *names, const int64_t *name_off, const char *suffix, int threads);
PCCX_API int pccx_ply_unpack(const void *staging, int64_t staging_bytes, const int64_t *table, const int32_t *tile_prefix, int B,
                             int64_t total_tiles, float *out, int64_t rows, void *stream);

/* ---- Point clouds sampled from triangle meshes (csrc/off_host.h, csrc/hostio.hip, csrc/mesh_sample.hip) ---------
 * Stands in for sample_modelnet.py's pyntcloud calls over a batch of OFF files: headers and bodies on host threads, the sampler on the
 * GPU.  The sampler is defined in DESIGN.md section 4.5 ("meshes") and is exact: integer area weights, Philox4x32-10, float64 points.
 * table (B, PCCX_OFF_ROW) int64 on the HOST, one row per file: 0 status (0 = good, else csrc/off_host.h OffStatus), 1 nv, 2 nf, 3 byte
 *   offset of the body, 4 file size, 5 ne, 6..7 zero.  msgs, paths, threads and the return value: as for the PLY pair above.
 * pccx_off_scan_host: opens every file, parses its header (limits: 3 <= nv <= 2^31 - 1, 1 <= nf <= 2^22, nv + nf shortest lines must
 *   fit the file) and fills its row.
 * pccx_off_load_host: for every row with status 0, the body parsed by its thread: nv * 3 float32 to staging_host + v_dst_off[b] and
 *   nf * 3 int32 indices local to the mesh to staging_host + f_dst_off[b] (both multiples of 4; one after the other per file, or all
 *   vertices in front of all faces, which is the packed form pccx_mesh_sample takes).  Refused: a polygon, an index outside 0 .. nv - 1,
 *   a coordinate that is no number or not finite as float32, fewer lines than nv + nf.  Nothing outside the two ranges is written.
 * pccx_mesh_sample (GPU): verts (V_total, 3) f32 and faces (F_total, 3) int32 packed mesh after mesh; v_off / f_off (B + 1) int64 ON THE
 *   DEVICE, the exclusive prefixes of nv and nf; seeds (B) int64 on the device, one 64-bit stream per mesh.  Writes out (B, n, 3) f32:
 *   row i of mesh b is a function of (mesh b, seeds[b], i) alone.  normalize = 1: (p - m) / M per mesh, m the minimum over its 3n
 *   values, M the maximum of p - m (sample_modelnet.py:47-48); 0: the raw samples.  status (B) int32: 0 good, 1 no area (largest
 *   triangle area zero or not finite, or a mesh outside the limits: its rows are NaN), 2 M == 0 (rows shifted, not scaled).
 *   Limits: B <= 1024, 1 <= n <= 2^20, F_b <= 2^22; every offset and index is clamped where it is read.  workspace: at least
 *   pccx_mesh_sample_workspace_bytes(B, F_total, n) bytes, 8-byte aligned, content immaterial; afterwards it begins with a_t (F_total
 *   float64), w_t (F_total uint64) and the inclusive prefix I_t (F_total uint64).  Six kernels and an init, integer atomics only, no
 *   memset / memcpy: capturable. */
#define PCCX_OFF_ROW 8
PCCX_API int pccx_off_scan_host(int B, const char *paths, const int64_t *path_off, int64_t *table, char *msgs, int msg_stride, int threads);
PCCX_API int pccx_off_load_host(int B, const char *paths, const int64_t *path_off, int64_t *table, void *staging_host,
                                int64_t staging_bytes, const int64_t *v_dst_off, const int64_t *f_dst_off, char *msgs, int msg_stride,
                                int threads);
PCCX_API size_t pccx_mesh_sample_workspace_bytes(int B, int64_t F_total, int n);
PCCX_API int pccx_mesh_sample(const float *verts, int64_t V_total, const int32_t *faces, int64_t F_total, const int64_t *v_off,
                              const int64_t *f_off, const int64_t *seeds, int B, int n, int normalize, float *out, int32_t *status,
                              void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCCX_H */
